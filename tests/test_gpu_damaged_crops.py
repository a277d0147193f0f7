"""Range, crop, ragged-crop and sample-crop calls on payloads that were damaged AFTER their index was written (include/ulc_amd.h
section 3).  The index is the clean stream's; one block of a file's bytes is not.  Every comparison is bit for bit (uint32 / int16
views of the samples, and d_bits) against tests/damage_testlib.py - the oracle's decoder run over the blocks of the row alone, each
cut to its index extent - and never against this library's own decode.  Outputs are poisoned before every call.
tests/test_damage_model.py checks the model and the damaged copies themselves on the CPU."""
import ctypes as C
import os
import numpy as np
import pytest

from gpu_testlib import amd as _amd, to_dev as _t
import damage_testlib as D
from ulc_testlib import same_bytes
from damage_testlib import blocks_of

pytestmark = pytest.mark.gpu
POISON_F, POISON_I = 7.0, 7
N = 4                                                       # blocks per row of the small calls
FMT = pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])


def _outputs(shape, nbits, pcm16):
    import torch
    pcm = torch.full(shape, POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full(nbits, POISON_I, dtype=torch.int32, device="cuda:0")
    return pcm, bits


def _crops(dec, cor, files, first, n_blocks, pcm16=False, ragged=False, keep=False, count=None):
    """ulcx_decode_crops(_ragged)_dev(_pcm16) on poisoned outputs -> (pcm [n][n_blocks][bs][ch], bits [n][n_blocks])."""
    import torch
    d, n = cor.to_device(), len(files)
    d_file, d_first = _t(files, np.int32), _t(first, np.int32)
    d_count = _t(count, np.int32) if count is not None else None
    cp = d_count.data_ptr() if d_count is not None else 0
    pcm, bits = _outputs((n, n_blocks, cor.bs, cor.ch), (n, n_blocks), pcm16)
    if ragged:
        dec.decode_crops_ragged_dev(cor.F, d["rpay"].data_ptr(), d["rpay"].numel(), d["poffs"].data_ptr(), d["idx"].data_ptr(), cor.F * cor.istride,
                                    d["ioffs"].data_ptr(), d["cnt"].data_ptr(), n, d_file.data_ptr(), d_first.data_ptr(), cp, n_blocks,
                                    pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    else:
        dec.decode_crops_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                             n, d_file.data_ptr(), d_first.data_ptr(), cp, n_blocks, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return (pcm, bits) if keep else (pcm.cpu().numpy(), bits.cpu().numpy())


def _range(dec, cor, first, n_blocks, pcm16=False):
    """ulcx_decode_range_dev(_pcm16): the corpus's files are the decoder's streams -> (pcm [F][n_blocks][bs][ch], bits [F][n_blocks])."""
    import torch
    d = cor.to_device()
    d_first = _t(first, np.int32)
    pcm, bits = _outputs((cor.F, n_blocks, cor.bs, cor.ch), (cor.F, n_blocks), pcm16)
    dec.decode_range_dev(d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                         d_first.data_ptr(), n_blocks, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _samples(dec, cor, files, start, n_samples, length=None, pcm16=False, ragged=False):
    """ulcx_decode_crops_samples(_ragged)_dev(_pcm16) on poisoned outputs -> (pcm [n][ch][n_samples], bits [n][nB])."""
    import torch
    d, n = cor.to_device(), len(files)
    d_file, d_start = _t(files, np.int32), _t(start, np.int64)
    d_len = _t(length, np.int32) if length is not None else None
    pcm, bits = _outputs((n, cor.ch, n_samples), (n, blocks_of(cor.bs, n_samples)), pcm16)
    lp = d_len.data_ptr() if d_len is not None else 0
    if ragged:
        dec.decode_crops_samples_ragged_dev(cor.F, d["rpay"].data_ptr(), d["rpay"].numel(), d["poffs"].data_ptr(), d["idx"].data_ptr(), cor.F * cor.istride,
                                            d["ioffs"].data_ptr(), d["cnt"].data_ptr(), n, d_file.data_ptr(), d_start.data_ptr(), lp, n_samples,
                                            pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    else:
        dec.decode_crops_samples_dev(cor.F, d["pay"].data_ptr(), cor.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                     n, d_file.data_ptr(), d_start.data_ptr(), lp, n_samples, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _differ(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    v = np.uint16 if g.dtype == np.int16 else np.uint32
    bad = np.argwhere(g.view(v) != w.view(v))
    return f"{len(bad)} of {w.size} samples differ from the model, first at {bad[0].tolist()}, last at {bad[-1].tolist()}"


def _check_crop_row(cor, f, first, n_blocks, pcm, bits, what, pcm16=False, count=None):
    """One row [n_blocks][bs][ch] against the model; beside the comparison: 0 bits and zero samples from the dead block on,
    positive sizes in front of it."""
    want, wb = cor.crop_row(f, first, n_blocks, count, pcm16)
    live = cor.model(f, first, n_blocks)[2] if count is None else min(cor.model(f, first, n_blocks)[2], max(0, int(count)))
    kind, j, sd = cor.files[f]
    where = f"{what}: file {f} ({kind}" + (f" of block {j}, seed {sd})" if j is not None else ")") + f" from block {first}"
    brow = np.asarray(bits)
    assert np.array_equal(brow, wb), f"{where}: bits {brow} vs the model's {wb}"
    assert (brow[:live] > 0).all() and (brow[live:] == 0).all(), f"{where}: bits {brow}, {live} blocks live"
    got = np.asarray(pcm).reshape(want.shape)
    assert not got[live:].any(), f"{where}: samples behind the row's end (block {first + live})"
    assert got.dtype == want.dtype and same_bytes(got, want), f"{where}: {_differ(got, want)}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. every geometry: the damage in every place of a row
# ---------------------------------------------------------------------------------------------------------------------
@FMT
@pytest.mark.parametrize("geom", D.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_damaged_block_in_every_place_of_a_row(geom, pcm16):
    """Per damaged file: the six rows of 4 blocks that hold its damaged block behind the row, as last, middle and first block, as
    the block in front, and in front of that; the same six rows of the clean file beside them; one row twice.  The strided and
    the ragged crop call, and the range call with the files as streams."""
    amd = _amd()
    bs, ch = geom
    cor = D.geometry_corpus(geom)
    pos = D.positions_of(geom)
    kinds = sorted({kd for kd, _, _ in cor.files})
    missing = [(kd, j) for j in pos for kd in ("draws", "resize") if not cor.of_kind(kd, j)]
    print(f"{cor.st.name}: {cor.F} files, damaged blocks {pos}, kinds {kinds}; no seed below {D.MAX_SEED} gives {missing or 'nothing less'}")
    for j in pos:
        assert cor.of_kind("kill", j) and cor.of_kind("value", j), f"{cor.st.name}: block {j} lacks a kill or a value damage"
    assert int(cor.st.wc[pos[-1]]) != 0x10 and cor.F <= 16
    dec = amd.BatchDecoder(16, ch, bs, N + 1)
    for f in range(1, cor.F):
        kind, j, _ = cor.files[f]
        around = [first for first, _ in D.rows_around(j)]
        files = [f] * 6 + [0] * 6 + [f]
        first = around + around + [around[3]]
        for ragged in (False, True):
            what = f"{'ragged' if ragged else 'strided'} crops around {kind} of block {j}"
            pcm, bits = _crops(dec, cor, files, first, N, pcm16, ragged)
            for i in range(len(files)):
                _check_crop_row(cor, files[i], first[i], N, pcm[i], bits[i], f"{what}, row {i}", pcm16)
            for i in (0, 5):                                # the damage behind the row / in front of the block in front: the clean file's row
                assert same_bytes(pcm[i], pcm[6 + i]) and np.array_equal(bits[i], bits[6 + i]), f"{what}: row {i} is not the clean file's"
            assert same_bytes(pcm[12], pcm[3]) and np.array_equal(bits[12], bits[3]), f"{what}: the row given twice"
            if kind == "kill":
                assert [int((bits[i] > 0).sum()) for i in range(6)] == [4, 3, 2, 0, 0, 4], f"{what}: {bits[:6]}"
            else:
                assert (bits[:12] > 0).all(), what
    # d_count: rows that are cut in front of the damaged block, at it and behind it
    for j in pos[1:]:
        kill, val = cor.of_kind("kill", j)[0], cor.of_kind("value", j)[0]
        files, first, count = [kill] * 5 + [val] * 5 + [0], [j - 2] * 10 + [j - 2], [0, 1, 2, 3, N + 2] * 2 + [3]
        for ragged in (False, True):
            pcm, bits = _crops(dec, cor, files, first, N, pcm16, ragged, count=count)
            for i in range(len(files)):
                _check_crop_row(cor, files[i], first[i], N, pcm[i], bits[i], f"{'ragged' if ragged else 'strided'} crops with counts, row {i}", pcm16, count[i])
            assert [int((bits[i] > 0).sum()) for i in range(11)] == [0, 1, 2, 2, 2, 0, 1, 2, 3, 4, 3], bits
    if not pcm16:                                           # the host form, once per geometry: every file with its damage in the middle
        files = list(range(cor.F))
        first = [(cor.files[f][1] or 6) - 2 for f in files]
        hp, hb = dec.decode_crops(cor.host, cor.nbytes, cor.index, cor.count, files, first, N)
        for i, f in enumerate(files):
            _check_crop_row(cor, f, first[i], N, hp[i], hb[i], f"host crops, row {i}")
    dec.close()
    # the range call: the files are the streams, stream f starts rel blocks from its own damaged block
    rdec = amd.BatchDecoder(cor.F, ch, bs, N + 1)
    at = np.array([cor.files[f][1] or 6 for f in range(cor.F)])
    clean = {}
    for rel in D.RELS + (-1,):
        first = at + rel
        pcm, bits = _range(rdec, cor, first, N, pcm16)
        for f in range(cor.F):
            _check_crop_row(cor, f, first[f], N, pcm[f], bits[f], f"range call {rel:+d} blocks from the damage", pcm16)
            if rel in (-4, 2):                              # untouched rows: byte-identical to the clean file's row from the same block
                if int(first[f]) not in clean:
                    clean[int(first[f])] = cor.crop_row(0, first[f], N, pcm16=pcm16)
                assert same_bytes(pcm[f], clean[int(first[f])][0]) and np.array_equal(bits[f], clean[int(first[f])][1]), (rel, f)
    if not pcm16:
        first = at - 2
        hp, hb = rdec.decode_range(cor.host, cor.nbytes, cor.index, cor.count, first, N)
        for f in range(cor.F):
            _check_crop_row(cor, f, first[f], N, hp[f], hb[f], "host range call")
    rdec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. sample crops
# ---------------------------------------------------------------------------------------------------------------------
SAMPLE_GEOMS = [(2048, 2), (4096, 2), (1024, 6), (1024, 2)]


def _sample_rows(cor, j, n_samples):
    """(files, start, length): starts an odd number of samples into the blocks j - 2 .. j + 2 of the file killed at block j (j - 1:
    the block in front of the dead one; j + 1: its block in front is dead), of a value-damaged file and of the clean one; one row
    twice.  Lengths end in front of block j, inside it and behind it."""
    bs = cor.bs
    kill = cor.of_kind("kill", j)[0]
    val = (cor.of_kind("draws", j) or cor.of_kind("value", j))[0]
    odd = (5, bs // 2 + 1, 1, bs - 1, bs // 4 - 1)
    files, start, length = [], [], []
    for f in (kill, val, 0):
        for i, b in enumerate(range(j - 2, j + 3)):
            s = b * bs + odd[i]
            to_j = j * bs - s                               # samples in front of block j (negative: the row starts in or behind it)
            files.append(f); start.append(s)
            length.append((to_j - 1, to_j + bs // 2 + 1, n_samples, to_j + 1, n_samples + 5)[i] if to_j > 0 else (bs // 2 + 1, n_samples, 3)[i - 2])
    files.append(kill); start.append(start[1]); length.append(length[1])
    return files, start, length


def _check_sample_rows(cor, files, start, n_samples, length, pcm, bits, what, pcm16):
    for i in range(len(files)):
        want, wb = cor.sample_row(files[i], start[i], n_samples, None if length is None else length[i], pcm16)
        kind, j, sd = cor.files[files[i]]
        where = f"{what}: row {i} (file {files[i]}, {kind} of block {j}, from sample {start[i]}" + (f", length {length[i]})" if length is not None else ")")
        assert np.array_equal(bits[i], wb), f"{where}: bits {bits[i]} vs the model's {wb}"
        assert pcm[i].dtype == want.dtype and same_bytes(pcm[i], want), f"{where}: {_differ(pcm[i], want)}"


@FMT
@pytest.mark.parametrize("geom", SAMPLE_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_sample_crops_around_a_dead_block(geom, pcm16):
    amd = _amd()
    bs, ch = geom
    cor = D.geometry_corpus(geom)
    n_samples = 2 * bs + 3
    dec = amd.BatchDecoder(16, ch, bs, blocks_of(bs, n_samples) + 1)
    for j in D.positions_of(geom)[1:]:                      # block 7 and the window-switched one
        files, start, length = _sample_rows(cor, j, n_samples)
        assert len(files) == 16
        for ragged in (False, True):
            for ln in (None, length):
                what = f"{'ragged' if ragged else 'strided'} sample crops around block {j}, {'with' if ln else 'without'} lengths"
                pcm, bits = _samples(dec, cor, files, start, n_samples, ln, pcm16, ragged)
                _check_sample_rows(cor, files, start, n_samples, ln, pcm, bits, what, pcm16)
                if ln is None:
                    # the killed file: rows from blocks j - 2 and j - 1 end with block j (zeros to the row's exact end), rows
                    # from j and j + 1 are silent, the row from j + 2 is the clean file's
                    to_j = [j * bs - s for s in start[:2]]
                    assert all((pcm[i][:, to_j[i]:] == 0).all() and pcm[i][:, :to_j[i]].any() for i in (0, 1)), what
                    assert [int((bits[i] > 0).sum()) for i in range(5)] == [2, 1, 0, 0, 4 if start[4] % bs + n_samples > 3 * bs else 3], f"{what}: {bits[:5]}"
                    assert not pcm[2].any() and not pcm[3].any() and same_bytes(pcm[4], pcm[14]), what
                    assert same_bytes(pcm[15], pcm[1]) and (bits[5:15, :3] > 0).all(), what
    if not pcm16:
        files, start, length = _sample_rows(cor, 7, n_samples)
        hp, hb = dec.decode_crops_samples(cor.host, cor.nbytes, cor.index, cor.count, files, start, n_samples, length=length)
        _check_sample_rows(cor, files, start, n_samples, length, hp, hb, "host form", False)
    dec.close()


@FMT
def test_sample_crops_of_a_dead_row_on_guarded_buffers(pcm16):
    """The planar clip stores of a dead block write zeros to the exact end of the row - every element over the poison - and not one
    sample further: d_pcm sits at an odd multiple of its element's size between guards, a plane has an odd number of samples."""
    import torch
    from test_gpu_sample_crops import _arena, _guarded_call, G_B, G_BS, G_CH, G_NS
    amd = _amd()
    cor = D.geometry_corpus((G_BS, G_CH))
    j = 7
    kill, val = cor.of_kind("kill", j)[0], (cor.of_kind("draws", j) or cor.of_kind("value", j))[0]
    files = [kill, kill, kill, kill, val, 0, kill, kill]
    start = [(j - 1) * G_BS + 1001, j * G_BS + 1, (j + 1) * G_BS + 3, (j - 2) * G_BS + 5, (j - 1) * G_BS + 1001, (j - 1) * G_BS + 1001, (j - 1) * G_BS + 1, j * G_BS - 1]
    length = [G_NS, G_NS, G_NS, G_NS, G_NS, G_NS, G_BS + 1, 2]        # (rows 6 and 7 end one sample into the dead block)
    n = len(files)
    assert n == G_B
    a = _arena(cor, n, pcm16)
    assert a.ptr("d_pcm") % (4 if pcm16 else 8) != 0
    a.load("d_file", np.array(files, np.int32)); a.load("d_start", np.array(start, np.int64)); a.load("d_len", np.array(length, np.int32))
    dec = amd.BatchDecoder(G_B, G_CH, G_BS, blocks_of(G_BS, G_NS) + 1)
    _guarded_call(dec, cor, a, n, pcm16)
    torch.cuda.synchronize()
    dec.close()
    a.check()
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, G_CH, G_NS)
    gbits = a.fetch("d_bits", np.int32).reshape(n, -1)
    _check_sample_rows(cor, files, start, G_NS, length, got, gbits, "guarded call", pcm16)
    assert got[0][:, :G_BS - 1001].any() and not got[0][:, G_BS - 1001:].any() and not got[1].any() and not got[2].any()
    assert got[6][:, :G_BS - 1].any() and not got[6][:, G_BS - 1:].any() and gbits[6, 0] > 0 and not gbits[6, 1:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. cut launches: the dead block in every position of a row
# ---------------------------------------------------------------------------------------------------------------------
def _tail_corpus():
    """Damages behind block 31 of the 40-block stream: in a row from block 0 or 1 they lie in the second 32-block chunk of a
    workgroup that walks the whole row."""
    return D.DamagedCorpus(D.stream_of(D.SWEEP_GEOM), [("kill", 33), ("value", 33), ("kill", 35), ("draws", 32), ("kill", 32), ("draws", 34)])


def _sweep(split):
    """Both sweep corpora and the tail corpus through one decoder created with ULCX_DSYN_SPLIT=split -> results keyed by call."""
    amd = _amd()
    bs, ch = D.SWEEP_GEOM
    old = os.environ.get("ULCX_DSYN_SPLIT")
    os.environ["ULCX_DSYN_SPLIT"] = split
    try:
        dec = amd.BatchDecoder(D.SWEEP_FILES, ch, bs, 37)
    finally:
        if old is None: os.environ.pop("ULCX_DSYN_SPLIT", None)
        else: os.environ["ULCX_DSYN_SPLIT"] = old
    resident = dec.last_cut()[2]
    out = {}
    for kind in ("kill", "value"):
        cor = D.sweep_corpus(kind)
        files = list(range(cor.F))
        for nb in (30, 36):
            out[kind, nb] = _crops(dec, cor, files, [1] * cor.F, nb)
            out[kind, nb, "cut"] = dec.last_cut()
        ns = 29 * bs + 1
        out[kind, "samples"] = _samples(dec, cor, files, [bs + 2 * f + 1 for f in files], ns)
        out[kind, "samples", "cut"] = dec.last_cut()
    tail = _tail_corpus()
    for first in (0, 1):
        out["tail", first] = _crops(dec, tail, list(range(tail.F)), [first] * tail.F, 36)
    dec.close()
    return resident, out


def test_dead_block_in_every_position_of_cut_and_uncut_rows():
    """31 files, file j killed at block j, one call of 31 rows x 30 blocks from block 1: under the even cut the dead block falls
    first, last and in the middle of a piece and in front of pieces that enter the row behind it; with the cut switched off one
    workgroup walks all 31 trips of a row (36-block rows: across the 32-block chunk).  The same with value damages (the generator
    moves at block j) and through the sample-crop call.  Both decoders against the model, and against each other."""
    amd = _amd()
    bs, ch = D.SWEEP_GEOM
    res1, cut = _sweep("1")
    res0, whole = _sweep("0")
    assert res1 > 0 and res0 == 0, (res1, res0)
    plan = amd.lib().ulcx_dec_split_plan(D.SWEEP_FILES, 30, res1)
    assert plan > D.SWEEP_FILES, f"31 rows x 30 blocks on {res1} resident workgroups: {plan} workgroups - no row is in pieces"
    for kind in ("kill", "value"):
        cor = D.sweep_corpus(kind)
        assert cut[kind, 30, "cut"][:2] == (plan, 0) and cut[kind, "samples", "cut"][:2] == (plan, 0), (cut[kind, 30, "cut"], cut[kind, "samples", "cut"])
        assert whole[kind, 30, "cut"][:2] == (0, 0) and whole[kind, 36, "cut"][:2] == (0, 0), whole[kind, 30, "cut"]
        for name, res in (("even cut", cut), ("one workgroup per row", whole)):
            for nb in (30, 36):
                pcm, bits = res[kind, nb]
                for f in range(cor.F):
                    _check_crop_row(cor, f, 1, nb, pcm[f], bits[f], f"{name}, {nb} blocks")
                if kind == "kill":
                    assert [int((bits[f] > 0).sum()) for f in range(cor.F)] == [max(0, f - 1) for f in range(cor.F)], name
            ns = 29 * bs + 1
            pcm, bits = res[kind, "samples"]
            files = list(range(cor.F))
            _check_sample_rows(cor, files, [bs + 2 * f + 1 for f in files], ns, None, pcm, bits, f"{name}, sample crops", False)
        for key in ((kind, 30), (kind, 36), (kind, "samples")):
            assert same_bytes(cut[key][0], whole[key][0]) and np.array_equal(cut[key][1], whole[key][1]), f"{key}: the two launch plans disagree"
    tail = _tail_corpus()
    assert [kd for kd, _, _ in tail.files] == ["clean", "kill", "value", "kill", "draws", "kill", "draws"]
    for name, res in (("even cut", cut), ("one workgroup per row", whole)):
        for first in (0, 1):
            pcm, bits = res["tail", first]
            for f in range(tail.F):
                _check_crop_row(tail, f, first, 36, pcm[f], bits[f], f"{name}, 36 blocks from {first}, damage in the second chunk")
            assert [int((bits[f] > 0).sum()) for f in (1, 3, 5)] == [33 - first, 35 - first, 32 - first], name


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cut of the last round
# ---------------------------------------------------------------------------------------------------------------------
def test_damaged_rows_in_whole_rounds_and_in_the_cut_round():
    """resident + 2 resident / 3 rows of 6 blocks drawn from the clean, killed and value-damaged files at seeded starts: whole
    rounds of one workgroup per row and a last round whose rows are cut into pieces (ulcx_dec_range_tail_plan)."""
    amd = _amd()
    geom = (2048, 2)
    bs, ch = geom
    cor = D.geometry_corpus(geom)
    nb = 6
    probe = amd.BatchDecoder(8, ch, bs, nb + 1)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    n = resident + resident * 2 // 3
    full = C.c_int32(0)
    tail = amd.lib().ulcx_dec_range_tail_plan(n, nb, resident, C.byref(full))
    assert tail > n - resident and full.value == resident, (n, resident, tail)
    rng = np.random.default_rng(41)
    files = rng.integers(0, cor.F, n).astype(np.int32)
    first = np.array([(cor.files[f][1] - rng.integers(-1, nb + 1)) if f else rng.integers(0, cor.K - nb) for f in files], np.int32)
    dec = amd.BatchDecoder(n, ch, bs, nb + 1)
    pcm, bits = _crops(dec, cor, files, first, nb, keep=True)
    grid, whole, _ = dec.last_cut()
    dec.close()
    assert (grid, whole) == (full.value + tail, full.value), (grid, whole, tail, full.value)
    rows = {0, 1, resident - 1, resident, resident + 1, resident + (n - resident) // 2, n - 2, n - 1}
    for lo, hi in ((0, resident), (resident, n)):           # and of each part the first two rows of every file
        for f in range(cor.F):
            rows |= set((lo + np.flatnonzero(files[lo:hi] == f)[:2]).tolist())
    kinds = {(cor.files[files[i]][0], i >= resident) for i in rows}
    assert {("clean", False), ("clean", True), ("kill", False), ("kill", True), ("value", False), ("value", True)} <= kinds, kinds
    dead = 0
    for i in sorted(rows):
        _check_crop_row(cor, int(files[i]), int(first[i]), nb, pcm[i].cpu().numpy(), bits[i].cpu().numpy(), f"row {i} of {n} ({resident} resident)")
        dead += cor.model(int(files[i]), int(first[i]), nb)[2] < nb
    assert dead >= 8, f"only {dead} of the {len(rows)} rows compared end at a dead block"
    # every row of the call: sizes against the model's (cheap), the samples of the rows above
    b = bits.cpu().numpy()
    for i in range(n):
        assert np.array_equal(b[i], cor.model(int(files[i]), int(first[i]), nb)[1]), f"row {i} (file {files[i]} from block {first[i]}): bits {b[i]}"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the state a range call leaves
# ---------------------------------------------------------------------------------------------------------------------
def test_state_after_a_range_call_over_damaged_streams():
    """Four streams - clean, killed at block 7, and two damaged at block 7 that live - take range calls of 3 blocks with block 7 as
    the last, the middle and the first block and as the block in front, each followed by decode_packed of 2 blocks.  A stream
    whose range held the kill reports 0 bits and zeros; the others go on as the model does when it runs two blocks further (the
    read position is the closing index entry of the range).  The next range call revives the dead stream."""
    amd = _amd()
    geom = (2048, 2)
    bs, ch = geom
    cor = D.geometry_corpus(geom)
    j = 7
    pick = [0, cor.of_kind("kill", j)[0], cor.of_kind("draws", j)[0], (cor.of_kind("resize", j) or cor.of_kind("value", j))[0]]
    host, nbytes = np.ascontiguousarray(cor.host[pick]), cor.nbytes[pick]
    index, count = np.ascontiguousarray(cor.index[pick]), cor.count[pick]
    dec = amd.BatchDecoder(4, ch, bs, N)
    n = N - 1
    for f0 in (j - 2, j - 1, j, j + 1, j + 2):
        first = np.full(4, f0, np.int32)
        pcm, bits = dec.decode_range(host, nbytes, index, count, first, n)
        nxt, nbits = dec.decode_packed(host, nbytes, 2)
        for s, f in enumerate(pick):
            what = f"stream {s} ({cor.files[f][0]}), range from block {f0}"
            _check_crop_row(cor, f, f0, n, pcm[s], bits[s], what)
            mp, mb, live = cor.model(f, f0, n + 2)
            if cor.model(f, f0, n)[2] < n:
                assert s == 1 and (nbits[s] == 0).all() and not nxt[s].any(), f"{what}: the packed call behind a dead range gives bits {nbits[s]}"
            else:
                assert live == n + 2
                assert np.array_equal(nbits[s], mb[n:]), f"{what}: the packed call behind it reports {nbits[s]}, the model {mb[n:]}"
                got = np.asarray(nxt[s], np.float32).reshape(2, bs, ch)
                assert same_bytes(got, mp[n:]), f"{what}: the packed call behind it: {_differ(got, mp[n:])}"
    dec.close()


def test_crop_calls_on_a_damaged_corpus_leave_every_streams_state_untouched():
    """A decoder half-way through decode_packed of four streams: crop, ragged-crop and sample-crop calls over the damaged corpus,
    dead rows among them, change no byte of any slot's saved record, and the clean streams go on as the oracle's."""
    amd = _amd()
    geom = (2048, 2)
    bs, ch = geom
    cor = D.geometry_corpus(geom)
    j = 7
    kill, val = cor.of_kind("kill", j)[0], cor.of_kind("draws", j)[0]
    pick = [0, val, kill, 0]
    host, nbytes = np.ascontiguousarray(cor.host[pick]), cor.nbytes[pick]
    dec = amd.BatchDecoder(4, ch, bs, N + 1)
    slots = list(range(4))
    p1, b1 = dec.decode_packed(host, nbytes, 3)
    before = dec.save_streams(slots)
    files, first = [kill, val, 0, kill], [j - 2, j - 1, j, j + 1]
    for ragged in (False, True):
        pcm, bits = _crops(dec, cor, files, first, N, ragged=ragged)
        for i in range(4):
            _check_crop_row(cor, files[i], first[i], N, pcm[i], bits[i], "crop call between two packed calls")
        assert before.tobytes() == dec.save_streams(slots).tobytes(), "a crop call changed a stream's state"
    ns = 2 * bs + 3
    start = [k * bs + 17 for k in first]
    pcm, bits = _samples(dec, cor, files, start, ns)
    _check_sample_rows(cor, files, start, ns, None, pcm, bits, "sample crops between two packed calls", False)
    assert before.tobytes() == dec.save_streams(slots).tobytes(), "a sample-crop call changed a stream's state"
    p2, b2 = dec.decode_packed(host, nbytes, 3)
    want, wb, _ = cor.model(0, 0, 6)
    for s in (0, 3):
        got = np.concatenate([np.asarray(p1[s], np.float32).reshape(3, bs, ch), np.asarray(p2[s], np.float32).reshape(3, bs, ch)])
        assert np.array_equal(np.concatenate([b1[s], b2[s]]), wb) and same_bytes(got, want), f"stream {s}: the packed decode around the crop calls"
    dec.close()
