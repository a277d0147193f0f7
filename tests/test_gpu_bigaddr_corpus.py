"""Corpus inputs beyond the 2^31- and 2^32-byte lines (tests/bigaddr_testlib.py): payload buffers and indexes of more than 4 GiB,
uninitialised but for a few files that lie below, across and above the lines, with a different valid file at every place a 32- or
31-bit form of a file's offset would point to.  Every decoder-side family reads them through the ragged layout, through a strided
layout of 4100 files and through one of three files 2^31 + 4096 bytes apart; every result is the oracle's, bit for bit
(corpus_testlib.File).  The premises - which file lies on which line, what lies at its aliases - are asserted without a GPU in
tests/test_bigaddr_capi.py, from the same planner."""
import numpy as np
import pytest

import bigaddr_testlib as B
import distortion_testlib as D
import splice_testlib as S
from bigaddr_testlib import REAL, STEREO
from corpus_testlib import INDEX_DTYPE, Corpus
from gpu_testlib import amd as _amd, to_dev as _t
from seek_testlib import SEED0
from ulc_testlib import to_pcm16

pytestmark = pytest.mark.gpu
PAY_SLACK, IDX_SLACK = 64 << 20, 16 << 20
N = 5                                                      # blocks per row
GEOMS = [(2048, 2), (1024, 1), (2048, 3)]
POISON_F, POISON_I = 7.0, 7


def _empty(nbytes):
    """nbytes of uninitialised device memory, or a skip that says how many."""
    import torch
    try:
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"no {nbytes} bytes of device memory: {str(e)[:120]}")


class View:
    """A corpus on the device as the calls take it: `args` is the run (nFiles, payload ... indexBlocks) of the layout's device forms,
    files {file number: File}; keep holds the tensors."""

    def __init__(self, ragged, args, files, keep):
        self.ragged, self.args, self.files, self.keep = ragged, args, files, keep
        self.sfx = "_ragged" if ragged else ""
        ref = next(iter(files.values()))
        self.bs, self.ch = ref.bs, ref.ch

    def rows(self):
        """Every file in at least two rows at different starts, a third for the long ones; one row past a file's end."""
        out = []
        for n, f in self.files.items():
            out += [(n, 0), (n, min(3, f.K - 1))] + ([(n, f.K - 4)] if f.K > 8 else [])
        return out + [(next(iter(self.files)), 10 ** 6)]


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_views():
    """The last view's buffers go back to the allocator before the next module runs."""
    yield
    import torch
    _cache.clear()
    torch.cuda.empty_cache()


def _one(key, build):
    """The view `key`, built once; only one view lives at a time (each holds several GiB)."""
    import torch
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache[key] = build()
    return _cache[key]


def _ragged_view(geom):
    def build():
        rb, _, _ = B.ragged_big(geom, REAL, PAY_SLACK, IDX_SLACK)
        pay, idx = _empty(rb.pay_total), _empty(8 * rb.idx_total)
        for at, b in rb.pay_pieces:
            pay[at:at + b.size] = _t(b)
        for at, r in rb.idx_pieces:
            idx[8 * at:8 * (at + r.size)] = _t(r.view(np.uint8))
        keep = (pay, idx, _t(rb.poffs), _t(rb.ioffs), _t(rb.blocks))
        args = (rb.F, pay.data_ptr(), rb.pay_total, keep[2].data_ptr(), idx.data_ptr(), rb.idx_total, keep[3].data_ptr(), keep[4].data_ptr())
        v = View(True, args, {2 * g: f for g, f in enumerate(rb.files)}, keep)
        v.rb = rb
        return v
    return _one(("ragged", tuple(geom)), build)


def _strided_view(kind):
    def build():
        m = B.strided_many(STEREO, REAL, 1 << B.MANY_STRIDE_LOG2, B.MANY_FILES, B.MANY_LIVE, B.MANY_DECOYS) if kind == "many" else B.strided_huge(STEREO, REAL)
        pay = _empty(m["stride"] * m["n_files"])
        for n, f in m["files"].items():
            pay[n * m["stride"]:n * m["stride"] + f.payload.size] = _t(f.payload)
        for at, f in m.get("decoy_at", {}).items():
            pay[at:at + f.payload.size] = _t(f.payload)
        keep = (pay, _t(m["nbytes"]), _t(m["index"].view(np.int32).reshape(m["n_files"], -1)), _t(m["blocks"]))
        args = (m["n_files"], pay.data_ptr(), m["stride"], keep[1].data_ptr(), keep[2].data_ptr(), m["istride"], keep[3].data_ptr())
        v = View(False, args, dict(m["files"]), keep)
        v.m = m
        return v
    return _one(("strided", kind), build)


def _view(layout, geom=STEREO):
    return _ragged_view(geom) if layout == "ragged" else _strided_view(layout)


def _out(shape, dtype):
    import torch
    return torch.full(shape, POISON_I if dtype in (torch.int16, torch.int32) else POISON_F, dtype=dtype, device="cuda:0")


def _same(got, want, what, rows):
    """got / want [n][...]: every bit; the first differing row is named with what it reads."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    n = got.shape[0]
    g, w = got.reshape(n, -1).view(np.uint8), want.reshape(n, -1).view(np.uint8)
    diff = B.first_diff(g, w, np.arange(n))
    assert diff is None, f"{what}: row {diff[0]} (file {rows[diff[0]][0]} from {rows[diff[0]][1]}) differs from the oracle's at byte {diff[1]} of the row"


LAYOUTS = ["ragged", "many", "huge"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. crops, float and int16
# ---------------------------------------------------------------------------------------------------------------------
def _crop_cases():
    return [(lay, STEREO) for lay in LAYOUTS] + [("ragged", g) for g in GEOMS[1:]]


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
@pytest.mark.parametrize("layout, geom", _crop_cases())
def test_crops_of_files_beyond_the_lines(layout, geom, pcm16):
    import torch
    v = _view(layout, geom)
    rows = v.rows()
    n = len(rows)
    dec = _amd().BatchDecoder(n, v.ch, v.bs, N + 1)
    pcm, bits = _out((n, N, v.bs, v.ch), torch.int16 if pcm16 else torch.float32), _out((n, N), torch.int32)
    d_file, d_first = _t([r[0] for r in rows], np.int32), _t([r[1] for r in rows], np.int32)
    getattr(dec, f"decode_crops{v.sfx}_dev")(*v.args, n, d_file.data_ptr(), d_first.data_ptr(), 0, N, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    dec.close()
    want = [v.files[f].expected_pcm(k, N) if k <= v.files[f].K else (np.zeros((N, v.bs, v.ch), np.float32), np.zeros(N, np.int32)) for f, k in rows]
    wp = np.stack([w[0] for w in want])
    assert all((w[1] > 0).any() for w in want[:-1]) and not want[-1][1].any()
    _same(bits.cpu().numpy(), np.stack([w[1] for w in want]), f"{layout} {geom}: d_bits", rows)
    _same(pcm.cpu().numpy(), to_pcm16(wp) if pcm16 else wp, f"{layout} {geom}: d_pcm", rows)


# ---------------------------------------------------------------------------------------------------------------------
# 2. sample crops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sample_crops_of_files_beyond_the_lines(layout):
    import torch
    amd = _amd()
    v = _view(layout)
    n_samples = 2 * v.bs + 1
    nB = amd.crop_blocks(v.bs, n_samples)
    rows = [(f, s) for f, file in v.files.items() for s in (1001, (file.K - 3) * v.bs + 77)]
    length = [n_samples if i % 3 else n_samples - 700 for i in range(len(rows))]
    n = len(rows)
    dec = amd.BatchDecoder(n, v.ch, v.bs, nB + 1)
    pcm, bits = _out((n, v.ch, n_samples), torch.float32), _out((n, nB), torch.int32)
    d_file, d_start, d_len = _t([r[0] for r in rows], np.int32), _t([r[1] for r in rows], np.int64), _t(length, np.int32)
    getattr(dec, f"decode_crops_samples{v.sfx}_dev")(*v.args, n, d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n_samples, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    dec.close()
    want = [B.sample_row(v.files[f], s, n_samples, ln) for (f, s), ln in zip(rows, length)]
    wb = np.zeros((n, nB), np.int32)
    for i, (_, b) in enumerate(want):
        wb[i, :len(b)] = b
    assert (wb[:, 0] > 0).all()
    _same(bits.cpu().numpy(), wb, f"{layout}: d_bits", rows)
    _same(pcm.cpu().numpy(), np.stack([w[0] for w in want]), f"{layout}: d_pcm", rows)


# ---------------------------------------------------------------------------------------------------------------------
# 3. spectra, both flags
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [0, 1], ids=["ms", "lr"])
@pytest.mark.parametrize("layout, geom", _crop_cases())
def test_spectra_of_files_beyond_the_lines(layout, geom, lr):
    import torch
    v = _view(layout, geom)
    rows = v.rows()[:-1]
    n = len(rows)
    dec = _amd().BatchDecoder(n, v.ch, v.bs, N + 1)
    coef, wc, bits = _out((n, v.ch, N, v.bs), torch.float32), _out((n, N), torch.int32), _out((n, N), torch.int32)
    d_file, d_first = _t([r[0] for r in rows], np.int32), _t([r[1] for r in rows], np.int32)
    getattr(dec, f"decode_crops_spectra{v.sfx}_dev")(*v.args, n, d_file.data_ptr(), d_first.data_ptr(), 0, N, lr, coef.data_ptr(), wc.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    dec.close()
    want = [v.files[f].expected_spec(k, N, None, bool(lr)) for f, k in rows]
    _same(wc.cpu().numpy(), np.stack([w[1] for w in want]), f"{layout} {geom}: d_wc", rows)
    _same(bits.cpu().numpy(), np.stack([w[2] for w in want]), f"{layout} {geom}: d_bits", rows)
    _same(coef.cpu().numpy(), np.stack([w[0] for w in want]), f"{layout} {geom}: d_coef", rows)


# ---------------------------------------------------------------------------------------------------------------------
# 4. distortion without a reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_distortion_of_files_beyond_the_lines(layout):
    import torch
    v = _view(layout)
    rows = v.rows()[:-1]
    n, n_seg = len(rows), 4
    numbers = list(v.files)
    model = Corpus([v.files[f] for f in numbers])           # the same files in a plain corpus, for the referee
    dec = _amd().BatchDecoder(n, v.ch, v.bs, N + 1)
    dist = torch.full((n, v.ch, N, n_seg, 3), POISON_F, dtype=torch.float64, device="cuda:0")
    wc, bits = _out((n, N), torch.int32), _out((n, N), torch.int32)
    d_file, d_first = _t([r[0] for r in rows], np.int32), _t([r[1] for r in rows], np.int32)
    getattr(dec, f"decode_crops_distortion{v.sfx}_dev")(*v.args, n, d_file.data_ptr(), d_first.data_ptr(), 0, N, 0, 0, 0, 0, 0, n_seg, 0,
                                                         dist.data_ptr(), wc.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    dec.close()
    wd, ww, wb = D.expected_rows(model, [numbers.index(f) for f, _ in rows], [k for _, k in rows], N, n_seg)
    assert (wd[..., 1] > 0).any()
    _same(wc.cpu().numpy(), ww, f"{layout}: d_wc", rows)
    _same(bits.cpu().numpy(), wb, f"{layout}: d_bits", rows)
    _same(dist.cpu().numpy().view(np.uint64), np.ascontiguousarray(wd).view(np.uint64), f"{layout}: d_dist", rows)


# ---------------------------------------------------------------------------------------------------------------------
# 5. splice with the high files as sources, and a crop decode of what it wrote
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splice_from_files_beyond_the_lines(layout):
    import torch
    v = _view(layout)
    numbers = list(v.files)
    src = S.source_of([v.files[f] for f in numbers])        # the referee's source: file g there is file numbers[g] here
    G = len(numbers)
    # output o: three blocks of every source file in turn, starting at o; then one output per source file alone
    model = [[((o + j) % G, 1 + j % 4, 3) for j in range(G)] for o in range(2)] + [[(g, 0, min(6, src.files[g].K))] for g in range(G)]
    device = [[(numbers[g], k, c) for g, k, c in f] for f in model]
    stride, istride = 3 * max(f.payload.size for f in src.files) + 37, 3 * G + 4
    exp, starts = S.expected(src, model, stride, istride)
    assert all(e.n == sum(c for _, _, c in f) for e, f in zip(exp, model))
    offs, seg = S.seg_arrays(device)
    n_out, n_seg = len(device), len(seg)
    d_offs, d_seg = _t(offs), _t(seg.view(np.int32))
    opay = torch.full((n_out, stride), 0xA5, dtype=torch.uint8, device="cuda:0")
    onb, omax, ocnt, ss = (_out((k,), torch.int32) for k in (n_out, n_out, n_out, n_seg))
    oidx = _out((n_out, 2 * istride), torch.int32)
    dec = _amd().BatchDecoder(n_out, v.ch, v.bs, 3 * G + 2)
    getattr(dec, f"corpus_splice{v.sfx}_dev")(*v.args, n_out, d_offs.data_ptr(), d_seg.data_ptr(), n_seg, opay.data_ptr(), stride, onb.data_ptr(), omax.data_ptr(),
                                              oidx.data_ptr(), istride, ocnt.data_ptr(), ss.data_ptr())
    nb = 3 * G
    pcm, bits = _out((n_out, nb, v.bs, v.ch), torch.float32), _out((n_out, nb), torch.int32)
    d_file, d_first = _t(np.arange(n_out), np.int32), _t(np.zeros(n_out), np.int32)
    dec.decode_crops_dev(n_out, opay.data_ptr(), stride, onb.data_ptr(), oidx.data_ptr(), istride, ocnt.data_ptr(), n_out, d_file.data_ptr(), d_first.data_ptr(), 0,
                         nb, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    dec.close()
    hpay, hidx = opay.cpu().numpy(), oidx.cpu().numpy().view(INDEX_DTYPE).reshape(n_out, istride)
    assert np.array_equal(ss.cpu().numpy(), starts)
    hp, hb = pcm.cpu().numpy(), bits.cpu().numpy()
    for o, e in enumerate(exp):
        what = f"{layout}: output {o} from {device[o]}"
        assert int(ocnt[o]) == e.n and int(onb[o]) == e.nbytes and int(omax[o]) == e.max_block, what
        assert hpay[o, :e.nbytes].tobytes() == e.payload.tobytes(), f"{what}: payload bytes differ from the source blocks'"
        assert (hpay[o, e.nbytes:] == 0xA5).all(), f"{what}: bytes behind the file written"
        assert hidx[o].tobytes() == e.index.tobytes(), f"{what}: index row differs from the oracle's walk"
        assert np.array_equal(hb[o, :e.n], e.bits) and not hb[o, e.n:].any() and hp[o, :e.n].tobytes() == e.pcm.tobytes() and not hp[o, e.n:].any(), \
            f"{what}: the crop decode of the output differs from the oracle's decode of the spliced blocks"


# ---------------------------------------------------------------------------------------------------------------------
# 6. the index calls: rows written at the high offsets, and nothing else
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_index_is_written_at_the_high_offsets():
    import torch
    v = _view("ragged")
    rb = v.rb
    idx = _empty(8 * rb.idx_total)
    words = idx.view(torch.int32)
    B.poison(words)
    cnt = _out((rb.F,), torch.int32)
    one = _amd().BatchDecoder(1, v.ch, v.bs, 2)
    one.index_packed_ragged_dev(rb.F, v.keep[0].data_ptr(), rb.pay_total, v.keep[2].data_ptr(), idx.data_ptr(), rb.idx_total, v.keep[3].data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    one.close()
    assert np.array_equal(cnt.cpu().numpy(), rb.blocks), (cnt.cpu().numpy(), rb.blocks)
    for g, (at, row) in enumerate(rb.idx_pieces):
        got = words[2 * at:2 * (at + row.size)].cpu().numpy().view(INDEX_DTYPE)
        bad = np.flatnonzero(got != row)
        assert bad.size == 0, f"file {2 * g} (row at entry {at}, byte {8 * at}): entries {bad[:6]} differ from the oracle's: {got[bad[:3]]} vs {row[bad[:3]]}"
    stray = B.still_poison(words, holes=[(2 * at, 2 * (at + row.size)) for at, row in rb.idx_pieces])
    assert stray is None, f"index word {stray} (byte {4 * stray}) outside every row was written"
    del idx, words
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", ["many", "huge"])
def test_strided_index_rows_of_files_beyond_the_lines(layout):
    import torch
    v = _view(layout)
    m = v.m
    F, istride = m["n_files"], m["istride"]
    idx, cnt = _out((F, 2 * istride), torch.int32), _out((F,), torch.int32)
    one = _amd().BatchDecoder(1, v.ch, v.bs, 2)
    one.index_packed_rows_dev(F, v.keep[0].data_ptr(), m["stride"], v.keep[1].data_ptr(), istride - 1, idx.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    one.close()
    want = m["index"].copy()
    want["RngState"][:, 0] = SEED0                          # (a file of no bytes: the open row)
    got = idx.cpu().numpy().view(INDEX_DTYPE).reshape(F, istride)
    assert np.array_equal(cnt.cpu().numpy(), m["blocks"]), np.flatnonzero(cnt.cpu().numpy() != m["blocks"])[:8]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{layout}: entries {bad[:4].tolist()} (file, entry) differ from the oracle's"


# ---------------------------------------------------------------------------------------------------------------------
# 7. a range decode of three streams 2^31 + 4096 bytes apart
# ---------------------------------------------------------------------------------------------------------------------
def test_range_decode_of_streams_a_huge_stride_apart():
    import torch
    v = _view("huge")
    m = v.m
    first = [1, 17, 30]
    dec = _amd().BatchDecoder(3, v.ch, v.bs, N + 1)
    pcm, bits = _out((3, N, v.bs, v.ch), torch.float32), _out((3, N), torch.int32)
    d_first = _t(first, np.int32)
    dec.decode_range_dev(v.keep[0].data_ptr(), m["stride"], v.keep[1].data_ptr(), v.keep[2].data_ptr(), m["istride"], v.keep[3].data_ptr(), d_first.data_ptr(), N,
                         pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    dec.close()
    want = [m["files"][s].expected_pcm(first[s], N) for s in range(3)]
    rows = list(zip(range(3), first))
    assert all((w[1] > 0).all() for w in want)
    _same(bits.cpu().numpy(), np.stack([w[1] for w in want]), "d_bits", rows)
    _same(pcm.cpu().numpy(), np.stack([w[0] for w in want]), "d_pcm", rows)
