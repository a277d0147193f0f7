"""Distortion on the GPU (include/ulc_amd.h section 3: ulcx_decode_crops_distortion_*): binary64 sums of the coded spectrum of crop
rows against caller-held reference planes.  Every comparison of sums is bit for bit (uint64 views) against the referee
(tests/distortion_testlib.py: numpy float64, separate * and -, the pairwise tree) on the oracle's coded coefficients
(tests/spectra_testlib.py); d_wc and d_bits against the oracle's.  The device calls run on poisoned buffers carved between guards
(tests/guarded_buffers.py), the reference planes among them.  What the inputs hold is asserted in tests/test_distortion_capi.py."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd, dev as _dev, word
import guarded_buffers as gb
import spectra_testlib as S
import distortion_testlib as T
import damage_testlib as D
from seek_testlib import oracle_pcm

pytestmark = pytest.mark.gpu
N = T.N_BLOCKS
LR = S.SPECTRA_LR
N_REF, N_RB = 3, N + 2                                     # reference rows and blocks per row of the row tests


def dist_dev(dec, lay, ch, bs, files, first, nb, n_seg, ref=None, ref_row=None, ref_first=None, count=None, flags=0, n_ref=None, n_rb=None):
    """One ulcx_decode_crops_distortion(_ragged)_dev call with every buffer - the reference planes and the two reference tables
    included - carved from a poisoned arena between guards -> (dist [n][ch][nb][n_seg][3], wc [n][nb], bits [n][nb]) after the
    guards and the inputs have been checked.  The outputs start as poison: what comes back equal to the referee was written.
    n_ref / n_rb: the counts handed to the call when they are not the planes' own."""
    import torch
    n = len(files)
    ragged = "poffs" in lay
    specs = [word("d_indexBlocks", len(lay["blocks" if ragged else "count"]), "in"), word("d_file", n, "in"), word("d_first", n, "in")]
    if ragged:
        specs += [dict(name="d_payload", nbytes=lay["payload"].size, align=1, role="in"),
                  dict(name="d_payloadOffs", nbytes=8 * lay["poffs"].size, align=8, role="in"),
                  dict(name="d_index", nbytes=8 * lay["index"].size, align=4, role="in"),
                  dict(name="d_indexOffs", nbytes=8 * lay["ioffs"].size, align=8, role="in")]
    else:
        specs += [dict(name="d_payload", nbytes=lay["host"].size, align=1, role="in", row=lay["host"].shape[1]), word("d_payloadBytes", lay["nbytes"].size, "in"),
                  dict(name="d_index", nbytes=8 * lay["index"].size, align=4, role="in")]
    for name, v in (("d_count", count), ("d_refRow", ref_row), ("d_refFirst", ref_first)):
        if v is not None:
            specs.append(word(name, n, "in"))
    if ref is not None:
        specs.append(dict(name="d_ref", nbytes=ref.nbytes, align=16, role="in", guard=4 * ref.shape[1] * ref.shape[2] * bs, row=4 * bs,
                          rows_per_stream=ref.shape[1] * ref.shape[2]))
    cell = 8 * 3 * n_seg
    specs += [dict(name="d_dist", nbytes=n * ch * nb * cell, align=8, role="out", guard=ch * nb * cell, row=cell, rows_per_stream=ch * nb),
              word("d_wc", n * nb, "out", rps=nb), word("d_bits", n * nb, "out", rps=nb)]
    a = gb.build(_dev(), specs)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32))
    for name, v in (("d_count", count), ("d_refRow", ref_row), ("d_refFirst", ref_first)):
        if v is not None:
            a.load(name, np.array(v, np.int64).astype(np.int32))
    if ref is not None:
        a.load("d_ref", ref)
    p = a.ptr
    opt = lambda name, v: p(name) if v is not None else 0
    tail = (n, p("d_file"), p("d_first"), opt("d_count", count), nb, opt("d_ref", ref),
            (ref.shape[0] if ref is not None else 0) if n_ref is None else n_ref, (ref.shape[2] if ref is not None else 0) if n_rb is None else n_rb,
            opt("d_refRow", ref_row), opt("d_refFirst", ref_first), n_seg, flags, p("d_dist"), p("d_wc"), p("d_bits"))
    if ragged:
        a.load("d_payload", lay["payload"]); a.load("d_payloadOffs", lay["poffs"]); a.load("d_index", lay["index"]); a.load("d_indexOffs", lay["ioffs"])
        a.load("d_indexBlocks", lay["blocks"])
        dec.decode_crops_distortion_ragged_dev(len(lay["blocks"]), p("d_payload"), lay["payload"].size, p("d_payloadOffs"), p("d_index"), lay["index"].size,
                                               p("d_indexOffs"), p("d_indexBlocks"), *tail)
    else:
        a.load("d_payload", lay["host"]); a.load("d_payloadBytes", lay["nbytes"]); a.load("d_index", lay["index"]); a.load("d_indexBlocks", lay["count"])
        dec.decode_crops_distortion_dev(lay["host"].shape[0], p("d_payload"), lay["host"].shape[1], p("d_payloadBytes"), p("d_index"), lay["index"].shape[1],
                                        p("d_indexBlocks"), *tail)
    torch.cuda.synchronize()
    a.check()
    return (a.fetch("d_dist", np.float64).reshape(n, ch, nb, n_seg, 3), a.fetch("d_wc", np.int32).reshape(n, nb), a.fetch("d_bits", np.int32).reshape(n, nb))


def spectra_planes(dec, cor, files, first, nb, count=None, flags=0):
    """ulcx_decode_crops_spectra_dev of the same rows -> (coef [n][ch][nb][bs], wc, bits) as numpy."""
    import torch
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(_dev())
    n = len(files)
    pay, nbytes, idx, cnt = t(cor.host), t(cor.nbytes), t(cor.index.view(np.int32).reshape(cor.index.shape[0], -1)), t(cor.count)
    d_file, d_first = t(np.array(files, np.int32)), t(np.array(first, np.int32))
    d_count = t(np.array(count, np.int32)) if count is not None else None
    coef = torch.full((n, cor.ch, nb, cor.bs), 7.0, dtype=torch.float32, device=_dev())
    wc = torch.full((n, nb), 7, dtype=torch.int32, device=_dev())
    bits = torch.full((n, nb), 7, dtype=torch.int32, device=_dev())
    dec.decode_crops_spectra_dev(cor.host.shape[0], pay.data_ptr(), cor.host.shape[1], nbytes.data_ptr(), idx.data_ptr(), cor.index.shape[1], cnt.data_ptr(),
                                 n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr() if d_count is not None else 0, nb, flags,
                                 coef.data_ptr(), wc.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    return coef.cpu().numpy(), wc.cpu().numpy(), bits.cpu().numpy()


def check(got, want, files, first, what):
    """dist, wc and bits of every row against the expected ones, bit for bit; the first row that differs is named."""
    for i in range(len(files)):
        where = f"{what}: row {i} (file {files[i]} from block {first[i]})"
        assert np.array_equal(got[2][i], want[2][i]), f"{where}: bits {got[2][i]} vs the oracle's {want[2][i]}"
        assert np.array_equal(got[1][i], want[1][i]), f"{where}: window codes {got[1][i]} vs {want[1][i]}"
        assert T.same_bits64(got[0][i], want[0][i]), f"{where}: sums differ at (channel, block, segment, sum; got; want) {T.first_diff(got[0][i], want[0][i])}"


def rows_of(cor, kind="table"):
    rows = S.seventy_rows(cor) if kind == "seventy" else S.row_table(cor)
    return [f for f, _ in rows], [k for _, k in rows]


# ---------------------------------------------------------------------------------------------------------------------
# 1. rows against the referee
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_count", [False, True], ids=["no-count", "count"])
@pytest.mark.parametrize("geom", T.geoms(), ids=lambda g: f"{g[0]}x{g[1]}")
def test_rows_equal_the_referee_on_the_oracles_coefficients(geom, with_count):
    """Every geometry - the stereo fast paths 2048 and 4096, mono, 3 and 6 channels, BlockSize 256 - at nSeg 1, 8 and 64 (64 at
    BlockSize 256: W = 4), against seeded reference planes with denormals, signed zeros and a wide range of exponents; every crop
    row i takes reference row i % 3, from reference block i % 3."""
    bs, ch = geom
    cor = T.corpus_of(geom)
    files, first = rows_of(cor)
    n = len(files)
    count = [(0, 1, N, N + 3)[i % 4] for i in range(n)] if with_count else None
    ref = T.ref_planes(N_REF, ch, N_RB, bs)
    ref_row, ref_first = [i % N_REF for i in range(n)], [i % 3 for i in range(n)]
    dec = _amd().BatchDecoder(n, ch, bs, N + 1)
    for n_seg in (1, 8, 64):
        got = dist_dev(dec, cor.strided(), ch, bs, files, first, N, n_seg, ref, ref_row, ref_first, count)
        want = T.expected_rows(cor, files, first, N, n_seg, ref, ref_row, ref_first, count)
        check(got, want, files, first, f"{bs} x {ch}, nSeg {n_seg}")
    assert dec.last_cut()[:2] == (0, 0)
    dec.close()
    live = want[1] != 0
    assert live.any() and (~live).any() and (want[0][..., 2] != want[0][..., 1]).any()


def test_seventy_rows_share_files_and_reference_rows():
    """More rows than a wave of the walk; d_refRow sends many crop rows to each of three reference rows; d_refFirst is NULL."""
    cor = S.geom_corpus((2048, 2))
    files, first = rows_of(cor, "seventy")
    n = len(files)
    ref = T.ref_planes(N_REF, 2, N_RB, 2048, seed=9)
    ref_row = [(i * 7) % N_REF for i in range(n)]
    dec = _amd().BatchDecoder(n, 2, 2048, N + 1)
    got = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, 16, ref, ref_row)
    check(got, T.expected_rows(cor, files, first, N, 16, ref, ref_row), files, first, "seventy rows")
    # d_refRow NULL: row i takes reference row i - rows 3 .. 69 have none
    got = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, 16, ref)
    want = T.expected_rows(cor, files, first, N, 16, ref)
    check(got, want, files, first, "seventy rows, d_refRow NULL")
    assert not want[0][3:, ..., 0].any() and want[0][:3, ..., 0].any()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference is the device's own output; no reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LR], ids=["ms", "lr"])
def test_against_its_own_spectra_the_error_is_zero(flags):
    cor = S.geom_corpus((2048, 3))
    files, first = rows_of(cor)
    n = len(files)
    dec = _amd().BatchDecoder(n, 3, 2048, N + 1)
    coef, wc, bits = spectra_planes(dec, cor, files, first, N, flags=flags)
    got = dist_dev(dec, cor.strided(), 3, 2048, files, first, N, 8, np.ascontiguousarray(coef), flags=flags)
    dec.close()
    assert np.array_equal(got[1], wc) and np.array_equal(got[2], bits)
    assert not got[0][..., 2].view(np.uint64).any(), "E is not +0.0 everywhere"
    assert T.same_bits64(got[0][..., 0], got[0][..., 1]) and got[0][..., 1].any()


@pytest.mark.parametrize("flags", [0, LR], ids=["ms", "lr"])
def test_without_a_reference_the_call_gives_the_coded_energies(flags):
    cor = S.geom_corpus((4096, 2))
    files, first = rows_of(cor)
    n = len(files)
    dec = _amd().BatchDecoder(n, 2, 4096, N + 1)
    coef, wc, bits = spectra_planes(dec, cor, files, first, N, flags=flags)
    got = dist_dev(dec, cor.strided(), 2, 4096, files, first, N, 32, None, flags=flags, n_ref=-5, n_rb=-7)     # (the counts: ignored without d_ref)
    dec.close()
    want = T.sums(np.zeros_like(coef), coef, 32)
    assert np.array_equal(got[1], wc) and np.array_equal(got[2], bits)
    assert not got[0][..., 0].view(np.uint64).any(), "S is not +0.0"
    assert T.same_bits64(got[0][..., 1], want[..., 1]) and T.same_bits64(got[0][..., 2], want[..., 1]) and want[..., 1].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. absent references
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_rows_and_blocks_outside_the_reference_count_as_zeros():
    """d_refRow of -1, nRef and INT32_MAX; d_refFirst leaving some, all or no block of a row outside [0, nRefBlocks), negative and so
    near INT32_MAX that the sum with the block number needs 64 bits.  Those blocks behave as a zero reference, the others are
    unaffected; the reference lies between guards and check() finds them untouched."""
    cor = S.geom_corpus((2048, 2))
    files, first = rows_of(cor, "seventy")
    n = len(files)
    ref = T.ref_planes(N_REF, 2, N_RB, 2048, seed=3)
    ref_row, ref_first = T.absent_tables(n, N_REF, N_RB)
    dec = _amd().BatchDecoder(n, 2, 2048, N + 1)
    got = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, 8, ref, ref_row, ref_first)
    want = T.expected_rows(cor, files, first, N, 8, ref, ref_row, ref_first)
    check(got, want, files, first, "absent references")
    out = T.outside(ref_row, ref_first, N_REF, N_RB)
    live = want[1] != 0
    S_ = got[0][..., 0]
    assert not S_.transpose(0, 2, 1, 3)[out].any() and S_.transpose(0, 2, 1, 3)[~out & live].all(axis=(-1, -2)).all()
    assert T.same_bits64(got[0][..., 2].transpose(0, 2, 1, 3)[out], got[0][..., 1].transpose(0, 2, 1, 3)[out])
    # the blocks without a reference are, in all three sums, those of the call without d_ref
    base = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, 8, None)
    assert T.same_bits64(got[0].transpose(0, 2, 1, 3, 4)[out], base[0].transpose(0, 2, 1, 3, 4)[out])
    dec.close()
    assert (out & live).sum() > 20 and (~out & live).sum() > 20


# ---------------------------------------------------------------------------------------------------------------------
# 4. LR; the largest block sizes; units of several noise passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (2048, 3), (1024, 6), T.SMALL], ids=lambda g: f"{g[0]}x{g[1]}")
def test_lr_sums_the_unmixed_pairs_and_leaves_a_single_channel(geom):
    bs, ch = geom
    cor = T.corpus_of(geom)
    files, first = rows_of(cor)
    n = len(files)
    ref = T.ref_planes(N_REF, ch, N_RB, bs, seed=5)
    ref_row = [i % N_REF for i in range(n)]
    dec = _amd().BatchDecoder(n, ch, bs, N + 1)
    n_seg = 64 if bs == 256 else 4
    got = dist_dev(dec, cor.strided(), ch, bs, files, first, N, n_seg, ref, ref_row, flags=LR)
    want = T.expected_rows(cor, files, first, N, n_seg, ref, ref_row, lr=True)
    check(got, want, files, first, f"{bs} x {ch}, LR")
    ms = dist_dev(dec, cor.strided(), ch, bs, files, first, N, n_seg, ref, ref_row)
    dec.close()
    for c in range(0, ch - 1, 2):
        assert not T.same_bits64(got[0][:, c], ms[0][:, c]) and not T.same_bits64(got[0][:, c + 1], ms[0][:, c + 1])
    if ch & 1:
        assert T.same_bits64(got[0][:, ch - 1], ms[0][:, ch - 1]) and ms[0][:, ch - 1, ..., 1].any()


@pytest.mark.parametrize("ch", [1, 2])
def test_blocksize_32768_takes_the_one_array_path_and_refuses_lr(ch):
    amd = _amd()
    cor = S.Corpus([S.big_stream(ch, True), S.big_stream(ch, False)] if ch == 1 else [S.big_stream(ch, True)])
    rows = [(f, k) for f in range(cor.F) for k in (0, 1)]
    files, first = [f for f, _ in rows], [k for _, k in rows]
    ref = T.ref_planes(2, ch, 3, 32768, seed=2)
    ref_row = [i % 2 for i in range(len(rows))]
    dec = amd.BatchDecoder(len(rows), ch, 32768, 3)
    for n_seg in (1, 2, 64):
        got = dist_dev(dec, cor.strided(), ch, 32768, files, first, 2, n_seg, ref, ref_row)
        check(got, T.expected_rows(cor, files, first, 2, n_seg, ref, ref_row), files, first, f"32768 x {ch}, nSeg {n_seg}")
    with pytest.raises(amd.UlcError, match=r"\(-1\).*ULCX_SPECTRA_LR at BlockSize 32768"):
        dist_dev(dec, cor.strided(), ch, 32768, files, first, 2, 1, ref, ref_row, flags=LR)
    dec.close()


def test_blocksize_16384_is_the_largest_with_lr():
    amd = _amd()
    from seek_testlib import oracle_stream
    blocks, bits, _ = oracle_stream(16384, 2, 30.0, 3, n_blocks=3)
    cor = S.Corpus([S.File("oracle 16384x2 q30", 16384, 2, blocks, bits)])
    files, first = [0, 0], [0, 1]
    ref = T.ref_planes(1, 2, 3, 16384, seed=4)
    dec = amd.BatchDecoder(2, 2, 16384, 3)
    for n_seg in (1, 64):
        got = dist_dev(dec, cor.strided(), 2, 16384, files, first, 2, n_seg, ref, [0, 0], [0, 1], flags=LR)
        check(got, T.expected_rows(cor, files, first, 2, n_seg, ref, [0, 0], [0, 1], lr=True), files, first, f"16384 x 2 LR, nSeg {n_seg}")
    dec.close()


def test_units_of_more_than_2048_noise_coefficients():
    cor = S.geom_corpus((4096, 2))
    rows = S.noise_pass_rows()
    files, first = [f for f, _ in rows], [k for _, k in rows]
    ref = T.ref_planes(N_REF, 2, N_RB, 4096, seed=6)
    ref_row = [i % N_REF for i in range(len(rows))]
    dec = _amd().BatchDecoder(len(rows), 2, 4096, N + 1)
    for flags in (0, LR):
        got = dist_dev(dec, cor.strided(), 2, 4096, files, first, N, 16, ref, ref_row, flags=flags)
        check(got, T.expected_rows(cor, files, first, N, 16, ref, ref_row, lr=bool(flags)), files, first, f"4096 x 2, flags {flags}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. damaged payloads
# ---------------------------------------------------------------------------------------------------------------------
def test_damaged_blocks_zero_the_sums_where_the_spectra_call_reports_no_block():
    """2048 x 2, block 7 of a file damaged behind its index - killed, value-damaged so that it still parses, resized so that the
    generator moves - and rows that have it in first, middle and last place and in front.  Expected: the referee on the oracle run
    block by block from the stored generator state (spectra_testlib.damaged_row); zeros exactly where wc is 0; behind a damaged block
    that still parses the sums follow the displaced noise."""
    st = D.stream_of((2048, 2))
    j = 7
    dc = D.DamagedCorpus(st, [("kill", j), ("value", j), ("draws", j)])
    kinds = [0, dc.of_kind("kill", j)[0], dc.of_kind("value", j)[0]] + list(dc.of_kind("draws", j))
    rows = [(f, k) for f in kinds for k in (j, j - 2, j - N + 1, j + 1)]       # the block first, in the middle, last, in front of the row
    files, first = [f for f, _ in rows], [k for _, k in rows]
    n = len(rows)
    coef, wc, bits = np.zeros((n, 2, N, 2048), np.float32), np.zeros((n, N), np.int32), np.zeros((n, N), np.int32)
    for i, (f, k) in enumerate(rows):
        coef[i], wc[i], bits[i], _ = S.damaged_row(dc.payloads[f], st.offs, st.seeds, 2, 2048, k, N)
    ref = T.ref_planes(N_REF, 2, N_RB, 2048, seed=8)
    ref_row = [i % N_REF for i in range(n)]
    want, _ = T.expected(coef, ref, ref_row, None, 8)
    want[np.broadcast_to((wc == 0)[:, None, :], want.shape[:3])] = 0.0
    lay = dict(host=dc.host, nbytes=dc.nbytes, index=dc.index, count=dc.count)
    dec = _amd().BatchDecoder(n, 2, 2048, N + 1)
    got = dist_dev(dec, lay, 2, 2048, files, first, N, 8, ref, ref_row)
    dec.close()
    check(got, (want, wc, bits), files, first, "damaged")
    dead = got[1] == 0
    assert not got[0].transpose(0, 2, 1, 3, 4)[dead].view(np.uint64).any() and got[0].transpose(0, 2, 1, 3, 4)[~dead][..., 1].any(axis=(-1, -2)).all()
    live = (~dead).sum(axis=1).reshape(len(kinds), 4)
    assert live[0].tolist() == [N] * 4 and live[1].tolist() == [0, 2, N - 1, 0] and live[2].tolist() == [N] * 4, live
    clean = got[0][:4]
    for g in range(3, len(kinds)):                          # a damage that moves the generator: the sums behind it follow the displaced noise
        assert not T.same_bits64(got[0][4 * g + 1][:, 3:], clean[1][:, 3:])


# ---------------------------------------------------------------------------------------------------------------------
# 6. nesting; layouts; host forms; refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(4096, 2), (512, 1), T.SMALL], ids=lambda g: f"{g[0]}x{g[1]}")
def test_the_device_sums_nest_from_64_segments_down_to_the_block(geom):
    bs, ch = geom
    cor = T.corpus_of(geom)
    files, first = rows_of(cor)
    files, first = files[:8], first[:8]
    ref = T.ref_planes(N_REF, ch, N_RB, bs, seed=12)
    ref_row = [i % N_REF for i in range(len(files))]
    dec = _amd().BatchDecoder(len(files), ch, bs, N + 1)
    d = dist_dev(dec, cor.strided(), ch, bs, files, first, N, 64, ref, ref_row)[0]
    n_seg = 64
    while n_seg > 1:
        n_seg //= 2
        d = T.halve(d)
        got = dist_dev(dec, cor.strided(), ch, bs, files, first, N, n_seg, ref, ref_row)[0]
        assert T.same_bits64(d, got), f"nSeg {n_seg}: {T.first_diff(d, got)}"
    dec.close()


@pytest.mark.parametrize("flags", [0, LR], ids=["ms", "lr"])
def test_ragged_entries_equal_the_strided_ones(flags):
    cor = S.geom_corpus((2048, 2))
    three = S.Corpus(cor.files + [cor.files[0]])
    rg = three.ragged()
    rg["poffs"][3] = rg["poffs"][2] - 1                     # file 2 is bytes [poffs[2], poffs[2] - 1): its rows have no block
    rows = S.row_table(cor) + [(2, 0), (2, 7), (0, 9), (1, 3)]
    files, first = [f for f, _ in rows], [k for _, k in rows]
    n = len(rows)
    count = [(N, N + 3, 1, N)[i % 4] for i in range(n)]
    ref = T.ref_planes(N_REF, 2, N_RB, 2048, seed=13)
    ref_row, ref_first = [i % N_REF for i in range(n)], [(i % 4) - 1 for i in range(n)]
    dec = _amd().BatchDecoder(n, 2, 2048, N + 1)
    got = dist_dev(dec, rg, 2, 2048, files, first, N, 16, ref, ref_row, ref_first, count, flags)
    seen = [-1 if f == 2 else f for f in files]
    check(got, T.expected_rows(cor, seen, first, N, 16, ref, ref_row, ref_first, count, lr=bool(flags)), files, first, "ragged")
    ok = [i for i, f in enumerate(files) if f != 2]
    pick = lambda v: [v[i] for i in ok]
    st = dist_dev(dec, cor.strided(), 2, 2048, pick(files), pick(first), N, 16, ref, pick(ref_row), pick(ref_first), pick(count), flags)
    dec.close()
    for j, i in enumerate(ok):
        assert T.same_bits64(st[0][j], got[0][i]) and np.array_equal(st[1][j], got[1][i]) and np.array_equal(st[2][j], got[2][i]), i
    bad = [i for i, f in enumerate(files) if f == 2]
    assert len(bad) == 2 and not got[0][bad].view(np.uint64).any() and not got[1][bad].any()


def test_host_forms_equal_the_device_forms_and_refuse_what_the_spectra_host_forms_refuse():
    amd = _amd()
    cor = S.geom_corpus((2048, 3))
    files, first = rows_of(cor)
    n = len(files)
    count = [(N, 2, N + 3, 0)[i % 4] for i in range(n)]
    ref = T.ref_planes(N_REF, 3, N_RB, 2048, seed=14)
    ref_row, ref_first = [(i % (N_REF + 1)) for i in range(n)], [(i % 3) - 1 for i in range(n)]
    dec = amd.BatchDecoder(n, 3, 2048, N + 1)
    rg = cor.ragged()
    for flags in (0, LR):
        dev = dist_dev(dec, cor.strided(), 3, 2048, files, first, N, 8, ref, ref_row, ref_first, count, flags)
        check(dev, T.expected_rows(cor, files, first, N, 8, ref, ref_row, ref_first, count, lr=bool(flags)), files, first, "device form")
        host = dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, files, first, N, ref, ref_row, ref_first, count=count, n_seg=8, flags=flags)
        check(host, dev, files, first, "host form")
        hr = dec.decode_crops_distortion_ragged(rg["payload"], rg["poffs"], rg["index"], rg["ioffs"], rg["blocks"], files, first, N, ref, ref_row, ref_first,
                                                count=count, n_seg=8, flags=flags)
        check(hr, dev, files, first, "ragged host form")
    none = dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, files, first, N, n_seg=8)
    check(none, dist_dev(dec, cor.strided(), 3, 2048, files, first, N, 8), files, first, "host form without a reference")
    K = cor.K[0]
    for hf, h1, hc, why in (([0, 1], [0, 0], None, "names file 1"), ([0, -1], [0, 0], None, "names file -1"), ([0, 0], [0, K + 1], None, "starts at block"),
                            ([0, 0], [0, -1], None, "starts at block"), ([0, 0], [0, 0], [1, -1], "wants -1 blocks")):
        with pytest.raises(amd.UlcError, match=why):
            dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, hf, h1, N, ref, count=hc)
        with pytest.raises(amd.UlcError, match=why):
            dec.decode_crops_distortion_ragged(rg["payload"], rg["poffs"], rg["index"], rg["ioffs"], rg["blocks"], hf, h1, N, ref, count=hc)
    falls = rg["poffs"].copy(); falls[1] = -4
    with pytest.raises(amd.UlcError, match="payload buffer"):
        dec.decode_crops_distortion_ragged(rg["payload"], falls, rg["index"], rg["ioffs"], rg["blocks"], [0], [0], N, ref)
    with pytest.raises(amd.UlcError, match="flags"):
        dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], N, ref, flags=2)
    with pytest.raises(amd.UlcError, match="nSeg"):
        dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], N, ref, n_seg=3)
    with pytest.raises(amd.UlcError, match="nBlocks"):
        dec.decode_crops_distortion(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], N + 1, ref)
    dec.close()


def test_every_refusal_returns_err_arg_with_the_outputs_untouched():
    import torch
    amd = _amd()
    cor = S.geom_corpus((2048, 2))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(_dev())
    pay, nbytes, idx, cnt = t(cor.host), t(cor.nbytes), t(cor.index.view(np.int32).reshape(cor.F, -1)), t(cor.count)
    d_file, d_first = t(np.array([0, 1, 0], np.int32)), t(np.array([3, 0, 9], np.int32))
    rows = t(np.array([0, 1, 0, 0], np.int32))
    host_ref = T.ref_planes(2, 2, N, 2048, seed=15)
    ref = t(np.concatenate([host_ref.reshape(-1), np.zeros(8, np.float32)]))
    n_seg = 8
    dist = torch.full((2 * 2 * N * n_seg * 3 + 4,), 7.0, dtype=torch.float64, device=_dev())
    wc = torch.full((2 * N + 2,), 7, dtype=torch.int32, device=_dev())
    bits = torch.full((2 * N + 2,), 7, dtype=torch.int32, device=_dev())
    dec = amd.BatchDecoder(2, 2, 2048, N + 1)

    def call(n=2, ro=0, n_ref=2, n_rb=N, rro=0, rfo=0, seg=n_seg, flags=0, do=0, wo=0, bo=0, with_ref=True):
        dec.decode_crops_distortion_dev(cor.F, pay.data_ptr(), cor.stride, nbytes.data_ptr(), idx.data_ptr(), cor.istride, cnt.data_ptr(), n, d_file.data_ptr(),
                                        d_first.data_ptr(), 0, N, ref.data_ptr() + ro if with_ref else 0, n_ref, n_rb, rows.data_ptr() + rro, rows.data_ptr() + rfo,
                                        seg, flags, dist.data_ptr() + do, wc.data_ptr() + wo, bits.data_ptr() + bo)
    for kw, why in ((dict(do=4), "d_dist.*not aligned"), (dict(ro=4), "d_ref.*not aligned"), (dict(ro=8), "d_ref.*not aligned"),
                    (dict(rro=2), "d_refRow.*not aligned"), (dict(rfo=1), "d_refFirst.*not aligned"), (dict(wo=2), "d_wc.*not aligned"),
                    (dict(bo=1), "d_bits.*not aligned"), (dict(n_ref=0), "nRef 0"), (dict(n_rb=0), "nRefBlocks 0"), (dict(n_ref=-1), "nRef -1"),
                    (dict(flags=LR | 4), "flags"), (dict(flags=2), "flags"), (dict(n=3), "n 3")) + tuple(
                        (dict(seg=s), "nSeg") for s in (0, -1, 3, 12, 128, 1024)):
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + why):
            call(**kw)
    small = amd.BatchDecoder(1, 1, 256, 2)                  # BlockSize / nSeg >= 4: 256 takes 64, and 128 is past the limit anyway
    with pytest.raises(amd.UlcError, match=r"\(-1\).*NULL"):
        small.decode_crops_distortion_dev(cor.F, pay.data_ptr(), cor.stride, nbytes.data_ptr(), idx.data_ptr(), cor.istride, cnt.data_ptr(), 1, d_file.data_ptr(),
                                          d_first.data_ptr(), 0, 1, 0, 0, 0, 0, 0, 64, 0, 0, wc.data_ptr(), bits.data_ptr())
    small.close()
    torch.cuda.synchronize()
    assert (dist == 7.0).all() and (wc == 7).all() and (bits == 7).all(), "a refused call wrote"
    call()
    call(with_ref=False, n_ref=0, n_rb=0)                   # (no reference: the counts are not looked at)
    call()
    torch.cuda.synchronize()
    want = T.expected_rows(cor, [0, 1], [3, 0], N, n_seg, host_ref, [0, 1], [0, 1])       # (both tables are `rows`)
    m = 2 * 2 * N * n_seg * 3
    got = (dist[:m].cpu().numpy().reshape(2, 2, N, n_seg, 3), wc[:2 * N].cpu().numpy().reshape(2, N), bits[:2 * N].cpu().numpy().reshape(2, N))
    check(got, want, [0, 1], [3, 0], "valid call behind the refused ones")
    assert (dist[m:] == 7.0).all() and (wc[2 * N:] == 7).all() and (bits[2 * N:] == 7).all()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the object's state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_streaming_decode_continues_across_distortion_calls_and_a_sample_crop_behind_one_is_unaffected():
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
    files, first = rows_of(cor)
    files, first = files[:B], first[:B]
    ref = T.ref_planes(N_REF, ch, N_RB, bs, seed=16)
    ref_row = [i % N_REF for i in range(B)]

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
        got = dist_dev(dec, cor.strided(), ch, bs, files, first, N, 8, ref, ref_row, flags=flags)
        check(got, T.expected_rows(cor, files, first, N, 8, ref, ref_row, lr=bool(flags)), files, first, "between two streaming calls")
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "a distortion call changed a stream's state"
    stream_call(1)
    dist_dev(dec, cor.strided(), ch, bs, files, first, N, 8, ref, ref_row)
    start, ns = [3 * bs + 100, 0, 20 * bs - 7], 2 * bs + 13
    pcm, _ = dec.decode_crops_samples(cor.host, cor.nbytes, cor.index, cor.count, [0, 1, 0], start, ns)
    for i, (f, st) in enumerate(zip([0, 1, 0], start)):
        flat = oracle_pcm(cor.files[f].blocks, ch, bs)[0].reshape(-1, ch)
        assert S.same_bits(pcm[i], flat[st:st + ns].T), f"sample crop row {i} behind a distortion call"
    stream_call(2)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. NaN and Inf in the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_in_the_reference_stay_inside_their_segment():
    cor = S.geom_corpus((2048, 2))
    files, first = [0, 0], [3, 9]
    ref = T.ref_planes(2, 2, N, 2048, seed=17)
    bad = ref.copy()
    n_seg, W = 16, 128
    spots = [(0, 0, 1, 5 * W + 3, np.nan), (0, 0, 1, 5 * W + 100, np.inf), (1, 1, 4, 15 * W + 127, -np.inf), (1, 0, 0, 0, np.nan)]
    for r, c, k, j, v in spots:
        bad[r, c, k, j] = v
    dec = _amd().BatchDecoder(2, 2, 2048, N + 1)
    clean = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, n_seg, ref)
    got = dist_dev(dec, cor.strided(), 2, 2048, files, first, N, n_seg, bad)
    dec.close()
    assert np.array_equal(got[1], clean[1]) and (clean[1] != 0).all()
    hit = np.zeros(got[0].shape[:4], bool)
    for r, c, k, j, _ in spots:
        hit[r, c, k, j // W] = True
    assert not np.isfinite(got[0][..., 0][hit]).any() and not np.isfinite(got[0][..., 2][hit]).any()
    assert T.same_bits64(got[0][..., 1], clean[0][..., 1]) and np.isfinite(got[0][..., 1]).all()
    assert T.same_bits64(got[0][~hit], clean[0][~hit])


# ---------------------------------------------------------------------------------------------------------------------
# 9. corpus.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["strided", "ragged"])
def test_crop_corpus_distortion_is_the_c_call(layout):
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
    files, first = rows_of(cor)
    n = len(files)
    count = [(N, 3, N + 3, 0)[i % 4] for i in range(n)]
    host_ref = T.ref_planes(N_REF, cor.ch, N_RB, cor.bs, seed=18)
    ref = torch.from_numpy(host_ref).to("cuda:0")
    ref_row, ref_first = [i % N_REF for i in range(n)], [(i % 3) for i in range(n)]
    dec = amd.BatchDecoder(n, cor.ch, cor.bs, N + 1)
    for lr in (False, True):
        dist, wc, bits = cc.distortion(dec, files, torch.tensor(first, dtype=torch.int32, device="cuda:0"), N, ref, ref_row, ref_first, count=count, n_seg=16, lr=lr)
        assert tuple(dist.shape) == (n, cor.ch, N, 16, 3) and dist.is_cuda and dist.dtype == torch.float64
        assert tuple(wc.shape) == tuple(bits.shape) == (n, N) and wc.dtype == bits.dtype == torch.int32
        torch.cuda.synchronize()
        got = (dist.cpu().numpy(), wc.cpu().numpy(), bits.cpu().numpy())
        check(got, T.expected_rows(cor, files, first, N, 16, host_ref, ref_row, ref_first, count, lr=lr), files, first, f"CropCorpus.distortion, {layout}")
        check(got, dist_dev(dec, cor.strided(), cor.ch, cor.bs, files, first, N, 16, host_ref, ref_row, ref_first, count, LR if lr else 0), files, first, "the C call")
    plain, _, _ = cc.distortion(dec, files, first, N)
    torch.cuda.synchronize()
    assert tuple(plain.shape) == (n, cor.ch, N, 1, 3) and not plain[..., 0].any() and torch.equal(plain[..., 1], plain[..., 2])
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. end to end: a ladder, its distortion, a plan, the switched corpus
# ---------------------------------------------------------------------------------------------------------------------
def test_a_ladders_distortion_plans_a_switch():
    import torch
    import corpus
    import clips_testlib as ct
    import clip_spectra_testlib as cs
    amd = _amd()
    bs, ch = 256, 2
    clips = list(range(1, 7))                               # six short clips: 1 .. 5 bs + 3 samples
    lengths = [ct.lengths(bs)[i] for i in clips]
    wave = ct.wave(bs, ch)[clips]
    nb = ct.clip_blocks(bs, ct.n_samples(bs))
    qs = (30.0, 70.0)
    enc = amd.BatchEncoder(len(clips), ch, bs, ct.RATE, 8)
    dec = amd.BatchDecoder(2 * len(clips), ch, bs, nb + 1)
    d_wave = torch.from_numpy(wave).to(_dev())
    cor = corpus.CropCorpus.from_clips_ladder(enc, dec, d_wave, lengths, rates=[(amd.MODE_VBR, q) for q in qs])
    clean, cwc, _ = corpus.clip_spectra(enc, d_wave, lengths)
    n = len(clips)
    by_rung = []
    # the referee: the oracle's encoder coefficients as the reference, the oracle's decode of the oracle's encode as the coded planes
    specs = [cs.row_spec(bs, ch, i) for i in clips]
    ref_np = cs.expected(specs, nb)[0]
    for r, q in enumerate(qs):
        dist, wc, bits = cor.distortion(dec, [cor.file_of(r, c) for c in range(n)], [0] * n, nb, clean, ref_row=list(range(n)), n_seg=8)
        torch.cuda.synchronize()
        coded = np.zeros((n, ch, nb, bs), np.float32)
        for c, i in enumerate(clips):
            cref = ct.ClipRef(bs, ch, ct.wave(bs, ch)[i][:, :lengths[c]], (-q, 0.0))
            f = S.File(f"clip {i} q{q:g}", bs, ch, cref.blocks, cref.bits)
            coded[c, :, :f.K] = f.coef.transpose(1, 0, 2)
            assert np.array_equal(wc[c, :f.K].cpu().numpy(), f.wc) and not wc[c, f.K:].any() and np.array_equal(cwc[c, :f.K].cpu().numpy(), f.wc)
        want, _ = T.expected(coded, ref_np, None, None, 8)
        want[np.broadcast_to((wc.cpu().numpy() == 0)[:, None, :], want.shape[:3])] = 0.0
        assert T.same_bits64(dist.cpu().numpy(), want), f"rung {r}: {T.first_diff(dist.cpu().numpy(), want)}"
        by_rung.append(dist)
    # a target between the rungs' block SNRs, taken from the data: some blocks reach it under the cheap rung, the others take the second
    d = torch.stack(by_rung).cpu()
    Ssum, Esum = d[..., 0].sum(dim=(2, 4)), d[..., 2].sum(dim=(2, 4))
    snr = torch.where(Esum == 0, torch.full_like(Ssum, float("inf")), 10.0 * torch.log10(Ssum / Esum))
    blocks = cor.d_index_blocks.cpu().numpy()[:n]
    live = torch.tensor([[k < blocks[c] for k in range(nb)] for c in range(n)])
    finite = snr[0][live & torch.isfinite(snr[0])]
    vals = torch.unique(finite)                             # (sorted)
    assert vals.numel() >= 8
    gaps = vals[1:] - vals[:-1]
    at = int(gaps[vals.numel() // 4: 3 * vals.numel() // 4].argmax()) + vals.numel() // 4
    target = float((vals[at] + vals[at + 1]) / 2)           # inside the widest gap of the middle half: no block's SNR is near it
    assert gaps[at] > 1e-6
    plan = corpus.rung_plan(by_rung, blocks, target)
    want_plan = corpus.rung_plan(d, blocks, target)
    assert plan == want_plan and [sum(m for _, m in row) for row in plan] == blocks.tolist()
    used = {r for row in plan for r, _ in row}
    assert used == {0, 1}, (target, plan)
    for c, row in enumerate(plan):
        k = 0
        for r, m in row:
            assert all((snr[0, c, k + j] >= target) == (r == 0) for j in range(m)), (c, row)
            k += m
    out = cor.switch(dec, plan)
    torch.cuda.synchronize()
    assert len(out) == n and out.d_index_blocks.cpu().tolist() == blocks.tolist()
    enc.close(); dec.close()
