"""Row outputs and caller buffers beyond the 2^31-byte, 2^32-byte and 2^31-element lines (tests/bigaddr_testlib.py): crop, int16
crop, sample-crop, spectra and synthesis calls of 16 392 and 32 776 rows of 16 stereo blocks of 2048, whose buffers measure
4 GiB + 2 MiB to 8 GiB + 2 MiB; a splice into 4100 outputs 2^20 bytes apart; a streaming encode and decode of 32 776 streams.
Row i names (file, first, count) = combos[rowmap[i]] of a table of some sixty combinations, planned so that two rows a line apart
- and neighbours - never name the same one; a few rows are short.  The output is poisoned on the device, and after the call
EVERY element of it is compared with table[rowmap] on the device, in chunks of rows, as integers: the table is the oracle's
(corpus_testlib.File, the oracle's encoder for the streams), a few tens of MB uploaded once.  Nothing is sampled and nothing is
compared GPU against GPU.  The plans' premises are asserted without a GPU in tests/test_bigaddr_capi.py.
The clips calls (32 776 clips of 32 768 samples into a 5 GiB corpus, with and without the spectra tap) and ulcx_corpus_ragged_dev
(more than 2^32 bytes back to back) are held to clips_testlib's and clip_spectra_testlib's oracle references in the same way."""
import numpy as np
import pytest

import bigaddr_testlib as B
from bigaddr_testlib import REAL
from gpu_testlib import amd as _amd, to_dev as _t
from ulc_testlib import to_pcm16

pytestmark = pytest.mark.gpu
BS, CH, N = 2048, 2, B.ROW_BLOCKS
ROW = N * BS * CH                                          # elements of a block-order row; CH * N * BS of a spectra row: the same


def _alloc(shape, dtype):
    """An uninitialised device tensor, or a skip that says how many bytes were asked for."""
    import torch
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    try:
        return torch.empty(shape, dtype=dtype, device="cuda:0")
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"no {nbytes} bytes of device memory: {str(e)[:120]}")


@pytest.fixture(scope="module")
def world():
    """The module's decoder of 32 776 streams x 17 blocks, the small corpus the rows read, and the oracle's tables on the device."""
    import torch
    amd = _amd()
    print("\ntorch.cuda.mem_get_info() at module start:", torch.cuda.mem_get_info())
    try:
        dec = amd.BatchDecoder(B.ROWS_8G, CH, BS, N + 1)
    except amd.UlcError as e:
        if "(-4)" not in str(e):
            raise
        pytest.skip(f"no device memory for a decoder of {B.ROWS_8G} streams x {N + 1} blocks (about 20 GiB of walk scratch): {e}")
    cor = B.rows_corpus()
    w = dict(dec=dec, cor=cor, d=cor.to_device(), tables={})
    yield w
    dec.close()
    w.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def wide(world):
    """The world with a decoder of 34 961 streams in place of its own: 32 776 rows put a 16-block float row past element 2^31, the
    channels-first rows of 15 x 2048 (+ 1) samples need 34 953 to get there.  (The streaming decode takes the object's own stream
    count, so it stays with the decoder of 32 776.)"""
    amd = _amd()
    try:
        dec = amd.BatchDecoder(B.ROWS_E31, CH, BS, N + 1)
    except amd.UlcError as e:
        if "(-4)" not in str(e):
            raise
        pytest.skip(f"no device memory for a decoder of {B.ROWS_E31} streams x {N + 1} blocks (about 22 GiB of walk scratch): {e}")
    yield dict(world, dec=dec)
    dec.close()


@pytest.fixture(scope="module")
def encoder(world):
    """The module's encoder of 32 776 streams x 17 blocks, shared by the clips and the streaming tests."""
    amd = _amd()
    try:
        enc = amd.BatchEncoder(B.ROWS_8G, CH, BS, 44100, N + 1)
    except amd.UlcError as e:
        if "(-4)" not in str(e):
            raise
        pytest.skip(f"no device memory for an encoder of {B.ROWS_8G} streams x {N + 1} blocks: {e}")
    yield enc
    enc.close()


def _table(w, kind, combos):
    """The expected rows of the combinations on the device, built once per kind: (rows as integers [T][row], bits [T][N], wc or None)."""
    key = (kind, len(combos))
    if key not in w["tables"]:
        files = B.rows_files()
        if kind in ("float", "pcm16"):
            tab, bits = B.pcm_table(files, combos, N)
            rows = to_pcm16(tab).view(np.int16) if kind == "pcm16" else tab.view(np.int32)
            wc = None
        else:
            tab, wc, bits = B.spec_table(files, combos, N, lr=kind == "lr")
            rows = tab.view(np.int32)
        w["tables"][key] = (_t(rows), _t(bits), None if wc is None else _t(wc))
    return w["tables"][key]


def _plan(n, esize):
    p = B.output_plan(n, ROW, esize, REAL)
    combos = np.array(p["combos"], np.int32)[p["rowmap"]]
    p["dev"] = tuple(_t(np.ascontiguousarray(combos[:, j])) for j in range(3))     # d_file, d_first, d_count
    p["rowmap_dev"] = _t(p["rowmap"])
    return p


def _poisoned(n, dtype):
    import torch
    out = _alloc((n, ROW), dtype)
    B.poison(out.view(torch.int32).reshape(-1))
    return out


def _check(out, table, p, shape, what):
    diff = B.first_diff(out, table, p["rowmap_dev"])
    assert diff is None, f"{what}: {B.name_diff(diff, shape, p['rowmap'], p['combos'])}"


def _check_words(got, table, p, what):
    """The small per-block outputs [n][N] against table[rowmap], whole."""
    diff = B.first_diff(got, table, p["rowmap_dev"], chunk=1 << 16)
    assert diff is None, f"{what}: {B.name_diff(diff, (N,), p['rowmap'], p['combos'])}"


def _crops(w, n, pcm16):
    import torch
    p = _plan(n, 2 if pcm16 else 4)
    tab, tbits, _ = _table(w, "pcm16" if pcm16 else "float", p["combos"])
    cor, d, dec = w["cor"], w["d"], w["dec"]
    out = _poisoned(n, torch.int16 if pcm16 else torch.float32)
    bits = torch.full((n, N), 7, dtype=torch.int32, device="cuda:0")
    d_file, d_first, d_count = p["dev"]
    dec.decode_crops_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                         n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), N, out.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    _check_words(bits, tbits, p, "d_bits")
    _check(out if pcm16 else out.view(torch.int32), tab, p, (N, BS, CH), "d_pcm16" if pcm16 else "d_pcm")
    del out
    torch.cuda.empty_cache()
    return p


def test_float_crops_across_the_byte_lines(world):
    """ulcx_decode_crops_dev, 16 392 rows: d_pcm is 4 GiB + 2 MiB and crosses 2^31 and 2^32 bytes."""
    p = _crops(world, B.ROWS_4G, False)
    assert sorted(p["on"]) == ["L31", "L32"]


def test_pcm16_crops_across_the_byte_and_element_lines(world):
    """ulcx_decode_crops_dev_pcm16, 32 776 rows: d_pcm16 is 4 GiB + 1 MiB of int16: 2^31 and 2^32 bytes, and element 2^31."""
    p = _crops(world, B.ROWS_8G, True)
    assert sorted(p["on"]) == ["E31", "L31", "L32"]


def test_spectra_across_every_line_both_flags_and_the_synthesis_of_those_planes(wide):
    """ulcx_decode_crops_spectra_dev, 34 961 rows: d_coef is 8.5 GiB; the verified planes are then the input of
    ulcx_synth_spectra_dev (_synth_from) and the reference of ulcx_decode_crops_distortion_dev (_distortion_against); the
    ULCX_SPECTRA_LR call goes to the same buffer, poisoned anew."""
    world = wide
    import torch
    n = B.ROWS_E31
    p = _plan(n, 4)
    assert sorted(p["on"]) == ["E31", "L31", "L32"]
    cor, d, dec = world["cor"], world["d"], world["dec"]
    d_file, d_first, d_count = p["dev"]
    out = _poisoned(n, torch.float32)
    for kind, flags in (("ms", 0), ("lr", 1)):
        tab, tbits, twc = _table(world, kind, p["combos"])
        if flags:
            B.poison(out.view(torch.int32).reshape(-1))
        wc = torch.full((n, N), 7, dtype=torch.int32, device="cuda:0")
        bits = torch.full((n, N), 7, dtype=torch.int32, device="cuda:0")
        dec.decode_crops_spectra_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                     n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), N, flags, out.data_ptr(), wc.data_ptr(), bits.data_ptr())
        torch.cuda.synchronize()
        _check_words(wc, twc, p, f"flags {flags}: d_wc")
        _check_words(bits, tbits, p, f"flags {flags}: d_bits")
        _check(out.view(torch.int32), tab, p, (CH, N, BS), f"flags {flags}: d_coef")
        if not flags:
            _synth_from(world, p, out, wc)
            _distortion_against(world, p, out)
    del out
    torch.cuda.empty_cache()


def _distortion_against(w, p, ref):
    """ulcx_decode_crops_distortion_dev of the plan's rows with d_ref = the planes the spectra call just wrote and the checker just
    verified (8.5 GiB across every line), d_refRow = bigaddr_testlib.ref_permutation: low rows read high reference rows and back.
    d_dist (1.7 GB, nSeg 64) is compared whole, as uint64, with distortion_testlib's referee on the distinct (row, reference row)
    combinations."""
    import torch
    import distortion_testlib as D
    n, n_seg = p["n"], 64
    perm = B.ref_permutation(n)
    pairs, pairmap = B.distinct_pairs(p["rowmap"], perm)
    assert (pairs[:, 0] != pairs[:, 1]).all() and len(pairs) <= 4 * p["T"]
    combos = [p["combos"][a] for a, _ in pairs]
    reftab = B.spec_table(B.rows_files(), p["combos"], N)[0].reshape(len(p["combos"]), CH, N, BS)
    wd, _, _ = D.expected_rows(w["cor"], [c[0] for c in combos], [c[1] for c in combos], N, n_seg, ref=reftab, ref_row=pairs[:, 1],
                               count=[c[2] for c in combos])
    tab = _t(np.ascontiguousarray(wd).reshape(len(pairs), -1).view(np.int64))
    cor, d, dec = w["cor"], w["d"], w["dec"]
    d_file, d_first, d_count = p["dev"]
    d_row = _t(perm, np.int32)
    dist = _alloc((n, CH * N * n_seg * 3), torch.float64)
    B.poison(dist.view(torch.int32).reshape(-1))
    wc, bits = (torch.full((n, N), 7, dtype=torch.int32, device="cuda:0") for _ in range(2))
    dec.decode_crops_distortion_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                    n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), N, ref.data_ptr(), n, N, d_row.data_ptr(), 0,
                                    n_seg, 0, dist.data_ptr(), wc.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    _, tbits, twc = _table(w, "ms", p["combos"])
    _check_words(wc, twc, p, "distortion d_wc")
    _check_words(bits, tbits, p, "distortion d_bits")
    diff = B.first_diff(dist.view(torch.int64), tab, _t(pairmap))
    if diff is not None:
        row, el = diff
        raise AssertionError(f"d_dist: row {row} {p['combos'][int(p['rowmap'][row])]} against reference row {int(perm[row])} "
                             f"{p['combos'][int(p['rowmap'][perm[row]])]}: first difference at {tuple(int(v) for v in np.unravel_index(el, (CH, N, n_seg, 3)))}")
    del dist
    torch.cuda.empty_cache()


def _synth_from(w, p, coef, wc):
    """ulcx_synth_spectra_dev with ULCX_SYNTH_WARM on planes the spectra call just wrote and the checker just verified (8 GiB + 2 MiB
    of input across every line): plane 0 of a row is the block in front, so the output [n][2][15 x 2048] (8 GiB + 1.9 MiB: 2^31 and
    2^32 bytes and element 2^31) is blocks first + 1 .. first + count - 1 of the row's file as a sample crop gives them, zeros behind."""
    import torch
    amd = _amd()
    n, n_out = p["n"], N - 1
    files = B.rows_files()
    rows, live = [], np.zeros((len(p["combos"]), n_out), np.int32)
    for j, (f, k, c) in enumerate(p["combos"]):
        rows.append(B.sample_row(files[f], (k + 1) * BS, n_out * BS, max(c - 1, 0) * BS)[0].reshape(-1))
        live[j, :max(c - 1, 0)] = 1
    tab, tlive = _t(np.stack(rows).view(np.int32)), _t(live)
    assert sorted(B.line_rows(n, CH * n_out * BS, {"E31": REAL.E31})) == ["E31"], "the output reaches element 2^31"
    pcm = _alloc((n, CH * n_out * BS), torch.float32)
    B.poison(pcm.view(torch.int32).reshape(-1))
    got_live = torch.full((n, n_out), 7, dtype=torch.int32, device="cuda:0")
    w["dec"].synth_spectra_dev(n, N, amd.SYNTH_WARM, coef.data_ptr(), wc.data_ptr(), pcm.data_ptr(), got_live.data_ptr())
    torch.cuda.synchronize()
    diff = B.first_diff(got_live, tlive, p["rowmap_dev"], chunk=1 << 16)
    assert diff is None, f"synth d_live: {B.name_diff(diff, (n_out,), p['rowmap'], p['combos'])}"
    diff = B.first_diff(pcm.view(torch.int32), tab, p["rowmap_dev"])
    assert diff is None, f"synth d_pcm: {B.name_diff(diff, (CH, n_out * BS), p['rowmap'], p['combos'])}"
    del pcm
    torch.cuda.empty_cache()


def test_sample_crops_across_every_line(wide):
    """ulcx_decode_crops_samples_dev, 34 961 rows of 15 x 2048 + 1 samples from unaligned starts: d_pcm [n][2][nSamples] is 8 GiB +
    2.2 MiB - 2^31 bytes, 2^32 bytes and element 2^31 each lie inside a row (a row is no multiple of anything)."""
    world = wide
    import torch
    amd = _amd()
    n, nS = B.ROWS_E31, B.SAMPLE_ROW
    nB = amd.crop_blocks(BS, nS)
    assert nB == N
    p = B.sample_plan(n, nS, CH, 4, REAL)
    assert sorted(p["on"]) == ["E31", "L31", "L32"]
    files = B.rows_files()
    tab, tbits = B.sample_table(files, p["combos"], nS, nB)
    tab, tbits = _t(tab.view(np.int32)), _t(tbits)
    combos = np.array(p["combos"], np.int64)[p["rowmap"]]
    d_file, d_start, d_len = _t(combos[:, 0], np.int32), _t(combos[:, 1], np.int64), _t(combos[:, 2], np.int32)
    p["rowmap_dev"] = _t(p["rowmap"])
    cor, d, dec = world["cor"], world["d"], world["dec"]
    out = _alloc((n, CH * nS), torch.float32)
    B.poison(out.view(torch.int32).reshape(-1))
    bits = torch.full((n, nB), 7, dtype=torch.int32, device="cuda:0")
    dec.decode_crops_samples_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                 n, d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), nS, out.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    _check_words(bits, tbits, p, "d_bits")
    diff = B.first_diff(out.view(torch.int32), tab, p["rowmap_dev"])
    assert diff is None, f"d_pcm: {B.name_diff(diff, (CH, nS), p['rowmap'], p['combos'])}"
    del out
    torch.cuda.empty_cache()


def test_streaming_encode_and_decode_beyond_element_2_31(world, encoder):
    """ulcx_encode_dev then ulcx_decode_dev, 32 776 streams x 16 blocks: 8 GiB + 2 MiB of PCM in and out - the first streaming call
    with an element index of 2^31 or more - and 4.3 GB of slots across 2^31 and 2^32 bytes.  Stream i is entry i mod T of a table of
    T distinct oracle-encoded streams; bytes (up to every block's size), sizes, WindowCtrl, BlockComplexity and the decoded PCM of
    EVERY stream are compared with the table on the device."""
    import torch
    from ulc_testlib import synth_pcm, oracle_encode_debug, oracle_decode_stream
    amd = _amd()
    n, K, rate = B.ROWS_8G, N, 44100
    slot = 2 * CH * BS + 16
    rowmap, T, on = B.stream_plan(n, [(ROW * 4, {"L31": REAL.L31, "L32": REAL.L32}), (ROW, {"E31": REAL.E31}), (K * slot, {"L31": REAL.L31, "L32": REAL.L32})])
    assert sorted(on[0]) == ["L31", "L32"] and sorted(on[1]) == ["E31"] and sorted(on[2]) == ["L31", "L32"]
    pcm = np.stack([synth_pcm(100 + t, K * BS, CH, rate, transient=True, seed=5) for t in range(T)])
    refs = [oracle_encode_debug(pcm[t], BS, rate, 0, 50.0, slot=slot) for t in range(T)]
    dec_ref = [oracle_decode_stream(r["out"], CH, BS) for r in refs]
    assert all(rc == 0 for rc, _, _ in dec_ref) and len({r["out"].tobytes() for r in refs}) == T
    nb = np.stack([(r["bits"] + 7) // 8 for r in refs]).astype(np.int32)
    assert (nb > 0).all() and (nb <= slot).all() and any((r["wc"] != 0x10).any() for r in refs)
    t_pcm, t_out, t_nb = _t(pcm.reshape(T, -1).view(np.int32)), _t(np.stack([r["out"] for r in refs])), _t(nb)
    t_bits, t_wc = _t(np.stack([r["bits"] for r in refs])), _t(np.stack([r["wc"] for r in refs]))
    t_cplx = _t(np.stack([r["cplx"] for r in refs]).view(np.int32))
    t_dec, t_dbits = _t(np.stack([p.reshape(-1) for _, p, _ in dec_ref]).view(np.int32)), _t(np.stack([b for _, _, b in dec_ref]))
    rm = _t(rowmap)
    p = dict(rowmap=rowmap, rowmap_dev=rm, combos=[(f"stream {t}",) for t in range(T)])
    enc, dec = encoder, world["dec"]
    assert enc.B == n and dec.B == n, "the streaming calls take the objects' own stream counts: the buffers below have n rows"
    enc.reset()
    assert enc.slot == slot
    d_in = _alloc((n, ROW), torch.int32)
    for a in range(0, n, 1024):                             # the input, gathered on the device: no multi-GiB array exists on the host
        d_in[a:a + 1024] = t_pcm[rm[a:a + 1024]]
    d_out = _alloc((n, K, slot), torch.uint8)
    B.poison(d_out.view(torch.int32).reshape(-1))
    bits, wc = (torch.full((n, K), 7, dtype=torch.int32, device="cuda:0") for _ in range(2))
    cplx = torch.full((n, K), 7.0, dtype=torch.float32, device="cuda:0")
    enc.encode_dev(d_in.data_ptr(), K, d_out.data_ptr(), bits.data_ptr(), wc.data_ptr(), cplx.data_ptr(), amd.MODE_VBR, 50.0)
    torch.cuda.synchronize()
    del d_in
    torch.cuda.empty_cache()
    for got, tab, what in ((bits, t_bits, "d_bits"), (wc, t_wc, "d_wc"), (cplx.view(torch.int32), t_cplx, "d_cplx")):
        diff = B.first_diff(got, tab, rm, chunk=1 << 16)
        assert diff is None, f"encode {what}: {B.name_diff(diff, (K,), rowmap, p['combos'])}"
    at = torch.arange(slot, device="cuda:0", dtype=torch.int32)
    for a in range(0, n, 512):                              # every byte of every block up to its size
        r = rm[a:a + 512]
        ne = (d_out[a:a + 512] != t_out[r]) & (at[None, None, :] < t_nb[r][:, :, None])
        if bool(ne.any()):
            s, k, byte = (int(v) for v in torch.nonzero(ne)[0])
            raise AssertionError(f"encode d_out: stream {a + s} (table entry {int(r[s])}) block {k}: byte {byte} differs from the oracle's")
    dec.reset()
    d_pcm = _alloc((n, ROW), torch.float32)
    B.poison(d_pcm.view(torch.int32).reshape(-1))
    dbits = torch.full((n, K), 7, dtype=torch.int32, device="cuda:0")
    dec.decode_dev(d_out.data_ptr(), slot, K, d_pcm.data_ptr(), dbits.data_ptr())
    torch.cuda.synchronize()
    diff = B.first_diff(dbits, t_dbits, rm, chunk=1 << 16)
    assert diff is None, f"decode d_bits: {B.name_diff(diff, (K,), rowmap, p['combos'])}"
    diff = B.first_diff(d_pcm.view(torch.int32), t_dec, rm)
    assert diff is None, f"decode d_pcm: {B.name_diff(diff, (K, BS, CH), rowmap, p['combos'])}"
    del d_pcm, d_out
    torch.cuda.empty_cache()


def test_splice_writes_4100_outputs_across_the_byte_lines(world):
    """ulcx_corpus_splice_dev, nOut = 4100 at an output payloadStride of 2^20: the new corpus is 4100 MiB.  Outputs 0, 2047, 2048,
    4095, 4096 and 4099 - below, at and above 2^31 and 2^32 bytes, 0 being where a 32-bit form of 4096's offset points - take
    different blocks; every other output has no segment.  Payload bytes, sizes, index rows and counts of the live outputs are
    splice_testlib's; every other byte of the 4100 MiB keeps its poison, every other row is an open, empty one."""
    import torch
    import splice_testlib as S
    from corpus_testlib import INDEX_DTYPE
    from seek_testlib import SEED0
    cor, d, dec = world["cor"], world["d"], world["dec"]
    src = S.source_of(cor.files)
    n_out, stride, istride = B.MANY_FILES, 1 << B.MANY_STRIDE_LOG2, 14
    live = {o: [(j % cor.F, 2 + j + 3 * (j % 2), 4), ((j + 1) % cor.F, j, 3)] for j, o in enumerate(B.MANY_LIVE)}
    segs = [live.get(o, []) for o in range(n_out)]
    exp, starts = S.expected(src, [live[o] for o in B.MANY_LIVE], stride, istride)
    assert all(e.n == 7 for e in exp) and len({e.payload.tobytes() for e in exp}) == len(exp)
    offs, seg = S.seg_arrays(segs)
    d_offs, d_seg = _t(offs), _t(seg.view(np.int32))
    opay = _alloc((n_out, stride), torch.uint8)
    words = opay.view(torch.int32).reshape(-1)
    words.fill_(0x5A5A5A5A)
    onb, omax, ocnt = (torch.full((n_out,), 7, dtype=torch.int32, device="cuda:0") for _ in range(3))
    ss = torch.full((len(seg),), 7, dtype=torch.int32, device="cuda:0")
    oidx = torch.full((n_out, 2 * istride), 7, dtype=torch.int32, device="cuda:0")
    dec.corpus_splice_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                          n_out, d_offs.data_ptr(), d_seg.data_ptr(), len(seg), opay.data_ptr(), stride, onb.data_ptr(), omax.data_ptr(),
                          oidx.data_ptr(), istride, ocnt.data_ptr(), ss.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ss.cpu().numpy(), starts)
    want_nb, want_cnt, want_max = (np.zeros(n_out, np.int32) for _ in range(3))
    want_idx = np.zeros((n_out, istride), INDEX_DTYPE)
    want_idx["ByteOffs"][:, 1:] = -1
    want_idx["RngState"][:, 0] = SEED0
    for o, e in zip(B.MANY_LIVE, exp):
        want_nb[o], want_cnt[o], want_max[o], want_idx[o] = e.nbytes, e.n, e.max_block, e.index
        got = opay[o, :e.nbytes].cpu().numpy()
        assert got.tobytes() == e.payload.tobytes(), f"output {o} (byte {o * stride} of the corpus): payload differs from the source blocks' at byte {int(np.flatnonzero(got != e.payload)[0])}"
        opay[o, :e.nbytes] = 0x5A                           # ... so that the whole buffer must be poison again
    for name, got, want in (("d_outPayloadBytes", onb, want_nb), ("d_outIndexBlocks", ocnt, want_cnt), ("d_outMaxBlock", omax, want_max)):
        bad = np.flatnonzero(got.cpu().numpy() != want)
        assert bad.size == 0, f"{name}: outputs {bad[:6]} hold {got.cpu().numpy()[bad[:6]]}, expected {want[bad[:6]]}"
    bad = np.argwhere(oidx.cpu().numpy().view(INDEX_DTYPE).reshape(n_out, istride) != want_idx)
    assert bad.size == 0, f"d_outIndex: (output, entry) {bad[:4].tolist()} differ"
    for a in range(0, words.shape[0], 1 << 26):
        ne = words[a:a + (1 << 26)] != 0x5A5A5A5A
        if bool(ne.any()):
            w = a + int(torch.nonzero(ne)[0])
            raise AssertionError(f"d_outPayload: byte {4 * w} (output {4 * w // stride}, offset {4 * w % stride}) was written outside every live output's bytes")
    del opay, words
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# clips: input [n][2][32 768] float (8 GiB + 2 MiB), a corpus of 32 776 files 160 KiB apart (5 GiB), planes [n][2][18][2048] (9 GiB)
# ---------------------------------------------------------------------------------------------------------------------
def _clips_world(w):
    """Plan, oracle references (clips_testlib.ClipRef, clip_spectra_testlib.SpecRef of the distinct clips) and their tables on the
    device, once per module."""
    import clips_testlib as ct
    import clip_spectra_testlib as cs
    if "clips" not in w:
        p = B.clips_plan(B.ROWS_8G, REAL)
        T, nb = p["T"], p["n_blocks"]
        waves = B.clip_waves(T)
        clips = [waves[t][:, :p["lengths"][t]] for t in range(T)]
        refs = [ct.ClipRef(BS, CH, c, ct.SCALAR) for c in clips]
        assert len({r.payload.tobytes() for r in refs}) == T and sorted({r.nb for r in refs}) == [0, 3, 8, nb]
        most = max(r.payload.size for r in refs)
        pay = np.zeros((T, most), np.uint8)
        for t, r in enumerate(refs):
            pay[t, :r.payload.size] = r.payload
        coef, wc, cplx = cs.expected([cs.SpecRef(BS, CH, c) for c in clips], nb)
        p.update(most=most, rm=_t(p["rowmap"]), t_in=_t(waves.reshape(T, -1).view(np.int32)), t_len=_t(p["lengths"].reshape(T, 1)), t_pay=_t(pay),
                 t_nb=_t(np.array([[r.payload.size] for r in refs], np.int32)), t_cnt=_t(np.array([[r.nb] for r in refs], np.int32)),
                 t_max=_t(np.array([[int(r.sizes.max()) if r.nb else 0] for r in refs], np.int32)),
                 t_idx=_t(np.stack([r.index_row(nb + 1) for r in refs]).view(np.int32).reshape(T, -1)),
                 t_coef=_t(coef.reshape(T, -1).view(np.int32)), t_wc=_t(wc), t_cplx=_t(cplx.view(np.int32)),
                 combos=[(f"clip {t}", int(p["lengths"][t])) for t in range(T)])
        w["clips"] = p
    return w["clips"]


def _named(p, diff, shape):
    return B.name_diff(diff, shape, p["rowmap"], p["combos"])


def _clips_call(w, enc, spectra):
    """ulcx_encode_clips_dev, or ulcx_encode_clips_spectra_dev, on 32 776 rows gathered on the device from the table of distinct
    clips; every output compared with the table, whole (payload: every byte of every file up to its size).  -> the corpus tensors."""
    import torch
    p = _clips_world(w)
    n, nb, rm, nS = p["n"], p["n_blocks"], p["rm"], B.CLIP_SAMPLES
    stride, istride = B.CLIP_STRIDE, nb + 1
    d_in = _alloc((n, CH * nS), torch.int32)
    for a in range(0, n, 1024):
        d_in[a:a + 1024] = p["t_in"][rm[a:a + 1024]]
    d_len = p["t_len"][rm].reshape(-1).contiguous()
    pay = _alloc((n, stride), torch.uint8)
    B.poison(pay.view(torch.int32).reshape(-1))
    nbytes, maxb, cnt = (torch.full((n, 1), 7, dtype=torch.int32, device="cuda:0") for _ in range(3))
    idx = torch.full((n, 2 * istride), 7, dtype=torch.int32, device="cuda:0")
    corpus = (pay.data_ptr(), stride, nbytes.data_ptr(), idx.data_ptr(), istride, cnt.data_ptr())
    if spectra:
        coef = _alloc((n, CH * nb * BS), torch.float32)
        B.poison(coef.view(torch.int32).reshape(-1))
        wc = torch.full((n, nb), 7, dtype=torch.int32, device="cuda:0")
        cplx = torch.full((n, nb), 7.0, dtype=torch.float32, device="cuda:0")
        enc.encode_clips_spectra_dev(w["dec"], n, d_in.data_ptr(), d_len.data_ptr(), nS, *corpus, nb, coef.data_ptr(), wc.data_ptr(), cplx.data_ptr(),
                                     d_max_block=maxb.data_ptr())
    else:
        enc.encode_clips_dev(w["dec"], n, d_in.data_ptr(), d_len.data_ptr(), nS, *corpus, d_max_block=maxb.data_ptr())
    torch.cuda.synchronize()
    del d_in
    torch.cuda.empty_cache()
    for got, tab, what in ((nbytes, p["t_nb"], "d_payloadBytes"), (cnt, p["t_cnt"], "d_indexBlocks"), (maxb, p["t_max"], "d_maxBlock"), (idx, p["t_idx"], "d_index")):
        diff = B.first_diff(got, tab, rm, chunk=1 << 16)
        assert diff is None, f"{what}: {_named(p, diff, (tab.shape[1],))}"
    at = torch.arange(p["most"], device="cuda:0", dtype=torch.int32)
    for a in range(0, n, 4096):
        r = rm[a:a + 4096]
        ne = (pay[a:a + 4096, :p["most"]] != p["t_pay"][r]) & (at[None, :] < p["t_nb"][r])
        if bool(ne.any()):
            i, byte = (int(v) for v in torch.nonzero(ne)[0])
            raise AssertionError(f"d_payload: file {a + i} (byte {(a + i) * stride} of the corpus; {p['combos'][int(r[i])]}): byte {byte} differs from the oracle's")
    if spectra:
        for got, tab, what in ((wc, p["t_wc"], "d_wc"), (cplx.view(torch.int32), p["t_cplx"], "d_cplx")):
            diff = B.first_diff(got, tab, rm, chunk=1 << 16)
            assert diff is None, f"{what}: {_named(p, diff, (nb,))}"
        diff = B.first_diff(coef.view(torch.int32), p["t_coef"], rm)
        assert diff is None, f"d_coef: {_named(p, diff, (CH, nb, BS))}"
        del coef
        torch.cuda.empty_cache()
    return pay, nbytes, idx, cnt


def test_clips_write_a_corpus_across_the_byte_lines_and_it_packs_beyond_2_32(world, encoder):
    """ulcx_encode_clips_dev: input across every line, the corpus it writes across 2^31 and 2^32 bytes.  Then ulcx_corpus_ragged_dev on
    that buffer with ragged_sizes() as d_payloadBytes (what lies behind a file's own bytes is the poison pattern: every byte of the
    5 GiB is known), so that the files lie back to back over more than 2^32 bytes: offsets, d_need, and every byte and entry of the
    output against the strided input."""
    import torch
    import clips_testlib as ct
    amd = _amd()
    pay, _, idx, cnt = _clips_call(world, encoder, False)
    p = world["clips"]
    n, stride, istride = p["n"], B.CLIP_STRIDE, p["n_blocks"] + 1
    sizes = B.ragged_sizes(n, stride)
    counts = cnt.reshape(-1).cpu().numpy()
    poffs, ioffs, blocks, need = ct.ragged_plan(sizes, stride, counts, istride, ct.NO_CAP, ct.NO_CAP)
    assert poffs[-1] == need[0] > REAL.L32 and (blocks == counts).all()
    d_sizes = _t(sizes)
    out = _alloc((int(need[0]),), torch.uint8)
    out.fill_(0xA5)
    oidx = torch.full((int(need[1]), 2), 7, dtype=torch.int32, device="cuda:0")
    d_po, d_io = (torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0") for _ in range(2))
    d_blocks = torch.full((n,), 7, dtype=torch.int32, device="cuda:0")
    d_need = torch.full((2,), -7, dtype=torch.int64, device="cuda:0")
    amd.corpus_ragged_dev(n, pay.data_ptr(), stride, d_sizes.data_ptr(), idx.data_ptr(), istride, cnt.data_ptr(), out.data_ptr(), int(need[0]), d_po.data_ptr(),
                          oidx.data_ptr(), int(need[1]), d_io.data_ptr(), d_blocks.data_ptr(), d_need.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_need.cpu().numpy(), need) and np.array_equal(d_blocks.cpu().numpy(), blocks)
    assert np.array_equal(d_po.cpu().numpy(), poffs) and np.array_equal(d_io.cpu().numpy(), ioffs)
    assert poffs[np.searchsorted(poffs, REAL.L32) - 1] < REAL.L32 and (poffs > REAL.L32).sum() > 100, "files start beyond 2^32 bytes"
    at = torch.arange(stride, device="cuda:0", dtype=torch.int32)
    ent = torch.arange(istride, device="cuda:0", dtype=torch.int32)
    idx64, oidx64 = idx.view(torch.int64), oidx.view(torch.int64).reshape(-1)
    for a in range(0, n, 2048):
        b = min(n, a + 2048)
        want = pay[a:b][at[None, :] < d_sizes[a:b, None]]                     # the files' bytes in order: what lies back to back
        ne = out[int(poffs[a]):int(poffs[b])] != want
        if bool(ne.any()):
            byte = int(poffs[a]) + int(torch.nonzero(ne)[0])
            f = int(np.searchsorted(poffs, byte, "right")) - 1
            raise AssertionError(f"d_outPayload: byte {byte} (file {f}, byte {byte - int(poffs[f])} of it) is not the strided file's")
        wante = idx64[a:b][ent[None, :] <= cnt[a:b]]
        ne = oidx64[int(ioffs[a]):int(ioffs[b])] != wante
        assert not bool(ne.any()), f"d_outIndex: entry {int(ioffs[a]) + int(torch.nonzero(ne)[0])} is not the strided row's"
    del out, pay
    torch.cuda.empty_cache()


def test_clip_spectra_planes_across_every_line(world, encoder):
    """ulcx_encode_clips_spectra_dev on the same rows: the planes [n][2][18][2048] (9 GiB) against the oracle's coef / wc / cplx, and the
    corpus byte-equal to the plain call's expectation."""
    import torch
    pay, _, _, _ = _clips_call(world, encoder, True)
    del pay
    torch.cuda.empty_cache()
