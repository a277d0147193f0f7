"""The plans and the checker of the address-line tests (tests/bigaddr_testlib.py) without a GPU: every premise a GPU test of
tests/test_gpu_bigaddr_*.py is named for - which line a file or a row lies on, which file lies at its alias - asserted from the
planner those tests call, and the evidence that they would fail on a narrow address: the same planner and checker at toy lines
(2^16 / 2^17 bytes, 2^15 elements) on numpy arrays, against stores and loads whose offsets are truncated to 32 bits, to 31 bits,
or sign-extended from 32 bits and clamped into the buffer.  No kernel is changed to show it."""
import numpy as np
import pytest

import bigaddr_testlib as B
from bigaddr_testlib import REAL, TOY, STEREO, WRAPS

GEOMS = [(2048, 2), (1024, 1), (2048, 3)]
TOY_PAY_SLACK, TOY_IDX_SLACK = 1 << 16, 1 << 13
REAL_PAY_SLACK, REAL_IDX_SLACK = 64 << 20, 16 << 20


# ---------------------------------------------------------------------------------------------------------------------
# 1. inputs: the placements
# ---------------------------------------------------------------------------------------------------------------------
def test_alias_arithmetic():
    h = 1 << 31
    assert B.aliases(5, h) == [] and B.aliases(h - 1, h) == []
    assert B.aliases(h + 5, h) == [5]                              # 31 bits; as a signed value it is negative
    assert B.aliases(2 * h + 5, h) == [5]                          # 32 bits unsigned, 31 bits and signed agree
    assert B.aliases(3 * h + 5, h) == [5, h + 5]
    assert B.wrap_s32(h + 5, h) == 5 - h and B.wrap_s32(h + 5, h, 100) == 0 and B.wrap_s32(2 * h + 500, h, 100) == 100


@pytest.mark.parametrize("lines, pslack, islack", [(TOY, TOY_PAY_SLACK, TOY_IDX_SLACK), (REAL, REAL_PAY_SLACK, REAL_IDX_SLACK)], ids=["toy", "real"])
@pytest.mark.parametrize("geom", GEOMS)
def test_ragged_placement_premises(geom, lines, pslack, islack):
    """Every role lies where its name says, in the payload buffer (bytes) and in the index (entries x 8 bytes); at every alias of a
    file's start another file starts, its content differs, and it is a valid file: the oracle decodes every block of it."""
    rb, pspans, ispans = B.ragged_big(geom, lines, pslack, islack)
    assert rb.pay_total == lines.L32 + pslack and 8 * rb.idx_total == lines.L32 + islack
    B.check_placement(pspans, lines.L31, rb.pay_total)
    B.check_placement({k.split(" ")[0]: v for k, v in ispans.items()}, lines.L31 // 8, rb.idx_total)
    by_start = {int(rb.poffs[2 * g]): rb.files[g] for g in range(rb.G)}
    rows_at = {int(rb.ioffs[2 * g]): g for g in range(rb.G)}
    n_alias = 0
    for g, f in enumerate(rb.files):
        assert (f.obits > 0).all() and f.pcm.shape == (f.K, f.bs, f.ch)             # valid: the oracle decodes it
        assert rb.blocks[2 * g] == f.K and rb.poffs[2 * g + 1] - rb.poffs[2 * g] == f.payload.size
        for a in B.aliases(int(rb.poffs[2 * g]), lines.L31):
            other = by_start[a]
            assert other is not f and other.payload.tobytes() != f.payload.tobytes()
            assert not np.array_equal(other.pcm[1:4], f.pcm[1:4]), "the alias decodes as the file itself"
            n_alias += 1
        for a in B.aliases(int(rb.ioffs[2 * g]), lines.L31 // 8):
            assert rows_at[a] != g and not np.array_equal(rb.idx_pieces[rows_at[a]][1], rb.idx_pieces[g][1])
            n_alias += 1
    assert n_alias >= 4
    # in-between files: falling payload offsets, so no walk starts on uninitialised bytes
    assert all(rb.poffs[f + 1] < rb.poffs[f] and rb.blocks[f] == 0 for f in range(1, rb.F, 2))
    assert (np.diff(rb.ioffs) >= 0).all()


def test_strided_placement_premises():
    m = B.strided_many(STEREO, REAL, 1 << B.MANY_STRIDE_LOG2, B.MANY_FILES, B.MANY_LIVE, B.MANY_DECOYS)
    st = m["stride"]
    assert st * B.MANY_FILES > REAL.L32 and 2047 * st < REAL.L31 == 2048 * st and 4095 * st < REAL.L32 == 4096 * st < 4099 * st
    assert sorted(m["files"]) == sorted(B.MANY_LIVE + B.MANY_DECOYS)
    idle = np.ones(B.MANY_FILES, bool); idle[list(m["files"])] = False
    assert (m["nbytes"][idle] == 0).all() and (m["blocks"][idle] == 0).all() and (m["nbytes"][~idle] > 0).all()
    assert B.aliases(4099 * st, REAL.L31) == [3 * st] and B.aliases(4096 * st, REAL.L31) == [0] and B.aliases(4095 * st, REAL.L31) == [2047 * st]
    h = B.strided_huge(STEREO, REAL)
    assert h["stride"] == REAL.L31 + 4096 and 3 * h["stride"] > REAL.L32 + REAL.L31
    for at, d in h["decoy_at"].items():
        assert h["files"][0].payload.size <= at and all(d.payload.tobytes() != f.payload.tobytes() for f in h["files"].values())
        assert (d.obits > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. outputs: the row plans the GPU tests run
# ---------------------------------------------------------------------------------------------------------------------
BS, CH, N = 2048, 2, B.ROW_BLOCKS
SAMPLES = 15 * BS + 1
OUTPUTS = {  # name: (rows, elements per row, bytes per element, lines it must cross)
    "crops float": (B.ROWS_4G, N * BS * CH, 4, ("L31", "L32")),
    "crops pcm16": (B.ROWS_8G, N * BS * CH, 2, ("L31", "L32", "E31")),
    "spectra": (B.ROWS_E31, CH * N * BS, 4, ("L31", "L32", "E31")),
}


@pytest.mark.parametrize("name", sorted(OUTPUTS))
def test_row_plan_premises(name):
    n, row, esize, crossed = OUTPUTS[name]
    p = B.output_plan(n, row, esize, REAL)
    assert sorted(p["on"]) == sorted(crossed), p["on"]
    rowmap, combos, n_full = p["rowmap"], p["combos"], p["n_full"]
    assert len(combos) == p["T"] <= 300
    units = {"L31": (row * esize, REAL.L31), "L32": (row * esize, REAL.L32), "E31": (row, REAL.E31)}
    for line, (a, b) in p["on"].items():
        u, L = units[line]
        assert a * u < L <= (a + 1) * u and b * u <= L < (b + 1) * u, "the rows that touch the line"
        for r in (a, b):
            assert combos[rowmap[r]][2] == N, f"row {r} on {line} is short"
        for d in {L // u, -(-L // u)}:
            assert (rowmap[d:] != rowmap[:-d]).all(), f"two rows {d} apart ({line}) name one combination"
    assert (rowmap[1:] != rowmap[:-1]).all()
    assert combos[rowmap[0]][2] == N and combos[rowmap[n - 1]][2] == N
    short = [i for i in range(n) if combos[rowmap[i]][2] < N]
    assert len(short) > 10 and all(0 <= combos[rowmap[i]][2] < N for i in short)
    files = B.rows_files()
    tab, bits = B.pcm_table(files, combos, N)
    assert len({t.tobytes() for t in tab}) == len(combos), "two combinations give one row"
    for j, (f, k, c) in enumerate(combos):
        assert (bits[j, :c] > 0).all() and (bits[j, c:] == 0).all() and not tab[j].reshape(N, -1)[c:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the checker against narrow stores, at the toy lines
# ---------------------------------------------------------------------------------------------------------------------
TOY_ROW = 64                                               # words per toy row: 256 bytes


def _toy_output():
    """1032 rows of 64 int32 words: 258 KiB, beyond 2^17 bytes and beyond 2 x 2^15 elements.  -> (plan, table int32 [T][64])"""
    n = 1032
    p = B.output_plan(n, TOY_ROW, 4, TOY)
    assert sorted(p["on"]) == ["E31", "L31", "L32"]
    tab, _ = B.pcm_table(B.rows_files(), p["combos"], N)
    toy = np.ascontiguousarray(tab.reshape(len(tab), N, -1)[:, :, 100:104].reshape(len(tab), TOY_ROW)).view(np.int32)
    assert len({t.tobytes() for t in toy}) == len(toy)
    return p, toy


def _stored(p, toy, wrap, unit):
    """The output a call leaves whose store offset of row i is wrap(i * row) in `unit` (1: elements against E31; 4: bytes against
    L31), clamped so that the row stays inside the buffer; wrap None: the right offset."""
    n = p["n"]
    words = np.zeros(n * TOY_ROW, np.int32)
    B.poison(words, chunk=1 << 12)
    half = TOY.L31 if unit == 4 else TOY.E31
    for i in range(n):
        o = i * TOY_ROW * unit
        if wrap is not None:
            o = wrap(o, half, (n - 1) * TOY_ROW * unit)
        assert 0 <= o <= (n - 1) * TOY_ROW * unit and o % unit == 0
        words[o // unit:o // unit + TOY_ROW] = toy[p["rowmap"][i]]
    return words.reshape(n, TOY_ROW)


def test_checker_accepts_the_right_output_and_names_one_wrong_word():
    p, toy = _toy_output()
    out = _stored(p, toy, None, 4)
    assert B.first_diff(out, toy, p["rowmap"], chunk=100) is None
    assert B.still_poison(out.reshape(-1), chunk=1 << 12) == 0
    for row, el in ((0, 0), (517, 63), (1031, 5)):
        bad = out.copy(); bad[row, el] ^= 1
        assert B.first_diff(bad, toy, p["rowmap"], chunk=100) == (row, el)
    words = np.zeros(5000, np.int32); B.poison(words, chunk=999)
    assert B.still_poison(words, chunk=777) is None and (words != 0).all()
    words[4321] = 0
    assert B.still_poison(words, chunk=777) == 4321 and B.still_poison(words, holes=[(4300, 4400)], chunk=777) is None


@pytest.mark.parametrize("unit", [4, 1], ids=["bytes", "elements"])
@pytest.mark.parametrize("model", sorted(WRAPS))
def test_checker_catches_a_narrow_store(model, unit, capsys):
    p, toy = _toy_output()
    out = _stored(p, toy, WRAPS[model], unit)
    got = B.first_diff(out, toy, p["rowmap"], chunk=100)
    want = np.argwhere(out != toy[p["rowmap"]])
    assert got is not None and got == tuple(int(v) for v in want[0]), (got, want[:1])
    half_rows = (TOY.L31 if unit == 4 else TOY.E31) // (TOY_ROW * unit)
    # the first wrong row is no later than the first row behind the line the model ends at: nothing hides behind it
    assert got[0] <= (half_rows if model != "u32" else 2 * half_rows), got
    # ... and the first row at the line the model ends at is itself seen wrong, where it belongs and where it landed
    r = half_rows if model != "u32" else 2 * half_rows
    landed = WRAPS[model](r * TOY_ROW * unit, TOY.L31 if unit == 4 else TOY.E31, (p["n"] - 1) * TOY_ROW * unit) // (TOY_ROW * unit)
    assert landed != r and (out[r] != toy[p["rowmap"][r]]).any() and (out[landed] != toy[p["rowmap"][landed]]).any(), (r, landed)
    behind = B.first_diff(out[r:], toy, p["rowmap"][r:], chunk=100)
    assert behind is not None and behind[0] == 0, "the checker, started at the line, names the row on it"
    with capsys.disabled():
        print(f"\n  narrow store {model} on {'bytes' if unit == 4 else 'elements'}: {B.name_diff(got, (TOY_ROW,), p['rowmap'], p['combos'])}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the checker against narrow loads, at the toy lines: a wrong but valid file
# ---------------------------------------------------------------------------------------------------------------------
def _toy_corpus():
    rb, _, _ = B.ragged_big(STEREO, TOY, TOY_PAY_SLACK, TOY_IDX_SLACK)
    pay = np.zeros(rb.pay_total, np.uint8)
    B.poison(pay.view(np.int32), chunk=1 << 12)
    for at, b in rb.pay_pieces:
        pay[at:at + b.size] = b
    idx = np.zeros(rb.idx_total, B.INDEX_DTYPE)
    for at, r in rb.idx_pieces:
        idx[at:at + r.size] = r
    return rb, pay, idx


def _loaded(rb, pay, idx, rows, n_blocks, wrap, what):
    """What a crop call gives whose offset of a file's payload (what = "payload", bytes) or of its index row (what = "index", bytes
    = 8 x entries) goes through `wrap`: it reads the index row and the bytes it finds there, and decodes as the oracle does when they are
    a file the corpus knows - a wrong but valid file.  -> float32 [n][n_blocks * bs * ch]"""
    known = {f.payload.tobytes(): f for f in rb.files}
    wrap = wrap or (lambda x, half, size: x)
    out = []
    for g, first in rows:
        p0, i0 = int(rb.poffs[2 * g]), int(rb.ioffs[2 * g])
        if what == "payload":
            p0 = wrap(p0, TOY.L31, rb.pay_total - 1)
        else:
            i0 = wrap(8 * i0, TOY.L31, 8 * (rb.idx_total - rb.cap)) // 8
        row = idx[i0:i0 + rb.cap]
        K = rb.files[g].K
        size = int(row["ByteOffs"][K]) if row["ByteOffs"][K] > 0 else 0
        f = known.get(pay[p0:p0 + size].tobytes())
        out.append(f.expected_pcm(first, n_blocks)[0].reshape(-1) if f is not None and size else np.zeros(n_blocks * rb.files[g].bs * rb.files[g].ch, np.float32))
    return np.stack(out)


@pytest.mark.parametrize("what", ["payload", "index"])
@pytest.mark.parametrize("model", [None] + sorted(WRAPS))
def test_checker_catches_a_narrow_load(model, what, capsys):
    rb, pay, idx = _toy_corpus()
    rows = [(g, k) for g in range(rb.G) for k in (0, 3)]
    nb = 5
    want = np.stack([rb.files[g].expected_pcm(k, nb)[0].reshape(-1) for g, k in rows]).view(np.int32)
    rowmap = np.arange(len(rows))
    got = _loaded(rb, pay, idx, rows, nb, WRAPS.get(model), what).view(np.int32)
    diff = B.first_diff(got, want, rowmap)
    if model is None:
        assert diff is None
        return
    assert diff is not None
    g, k = rows[diff[0]]
    at = int(rb.poffs[2 * g]) if what == "payload" else 8 * int(rb.ioffs[2 * g])
    assert at >= TOY.L31, "the first wrong row names a file at or above the first line"
    with capsys.disabled():
        print(f"\n  narrow load {model} of the {what}: row {diff[0]} (file {2 * g} at byte {at}, from block {k}) differs first, at element {diff[1]}")


def test_sample_row_plan_premises():
    """The large sample-crop output [34 961][2][15 x 2048 + 1] float32 is 8 GiB + 2.2 MiB: both byte lines and element 2^31 lie
    INSIDE a row (its length divides nothing), the rows on them are full length with unaligned starts; the synthesis output
    [34 961][2][15 x 2048] reaches element 2^31 too.  (32 776 rows, the count of the block-order outputs, stop at 2.01e9 elements.)"""
    n, nS = B.ROWS_E31, B.SAMPLE_ROW
    p = B.sample_plan(n, nS, CH, 4, REAL)
    row = CH * nS
    assert sorted(p["on"]) == ["E31", "L31", "L32"] and B.ROWS_8G * row < REAL.E31 < (n - 8) * row and n * row * 4 < (8 << 30) + (3 << 20)
    assert (n - 9) * CH * (nS - 1) < REAL.E31 < (n - 8) * CH * (nS - 1)
    for line, L, u in (("L31", REAL.L31, 4 * row), ("L32", REAL.L32, 4 * row), ("E31", REAL.E31, row)):
        a, b = p["on"][line]
        assert a == b and a * u < L < (a + 1) * u and L % u != 0
        f, start, ln = p["combos"][p["rowmap"][a]]
        assert ln == nS and start % BS != 0
    rowmap = p["rowmap"]
    for d in (1, REAL.L31 // (4 * row), REAL.L31 // (4 * row) + 1, REAL.L32 // (4 * row), REAL.L32 // (4 * row) + 1, REAL.E31 // row, REAL.E31 // row + 1):
        assert (rowmap[d:] != rowmap[:-d]).all()
    tab, bits = B.sample_table(B.rows_files(), p["combos"], nS, N)
    assert len({t.tobytes() for t in tab}) == len(tab)
    short = [c for c in p["combos"] if c[2] < nS]
    assert short and all(not tab[p["combos"].index(c)].reshape(CH, nS)[:, c[2]:].any() for c in short)
    assert all(s % BS for _, s, _ in p["combos"][:p["n_full"]]), "an aligned start among the full rows"


def test_streaming_plan_premises():
    """32 776 streams x 16 blocks: the PCM of the streaming calls crosses both byte lines and element 2^31 (the last element index is
    2^31 + 2^19 - 1), the slots cross both byte lines inside a stream's row; streams a line apart carry different table entries."""
    n, slot = B.ROWS_8G, 2 * CH * BS + 16
    row = N * BS * CH
    rowmap, T, on = B.stream_plan(n, [(row * 4, {"L31": REAL.L31, "L32": REAL.L32}), (row, {"E31": REAL.E31}), (N * slot, {"L31": REAL.L31, "L32": REAL.L32})])
    assert n * row - 1 == REAL.E31 + (1 << 19) - 1 and n * N * slot > REAL.L32
    assert sorted(on[0]) == ["L31", "L32"] and sorted(on[1]) == ["E31"] and sorted(on[2]) == ["L31", "L32"]
    a, b = on[2]["L32"]
    assert a == b and a * N * slot < REAL.L32 < (a + 1) * N * slot
    for d in (1, 8192, 16384, 32768, REAL.L31 // (N * slot), REAL.L31 // (N * slot) + 1, REAL.L32 // (N * slot), REAL.L32 // (N * slot) + 1):
        assert (rowmap[d:] != rowmap[:-d]).all(), d
    assert 16 < T <= 31 and rowmap.max() == T - 1


def test_checker_and_poison_agree_between_numpy_and_torch():
    """The GPU tests hand the same functions torch tensors: the pattern, the search for a stray word and the first difference are
    the same there (CPU tensors here)."""
    import torch
    p, toy = _toy_output()
    out = torch.from_numpy(_stored(p, toy, None, 4).copy())
    t_toy, t_map = torch.from_numpy(toy), torch.from_numpy(p["rowmap"])
    assert B.first_diff(out, t_toy, t_map, chunk=100) is None
    out[777, 13] ^= 1
    assert B.first_diff(out, t_toy, t_map, chunk=100) == (777, 13)
    bad = torch.from_numpy(_stored(p, toy, WRAPS["u31"], 4).copy())
    assert B.first_diff(bad, t_toy, t_map, chunk=100) == B.first_diff(bad.numpy(), toy, p["rowmap"], chunk=100) != None
    a, b = np.zeros(5000, np.int32), torch.zeros(5000, dtype=torch.int32)
    B.poison(a, chunk=999); B.poison(b, chunk=1024)
    assert np.array_equal(a, b.numpy()) and B.still_poison(b, chunk=777) is None
    b[4321] = 0
    assert B.still_poison(b, chunk=777) == 4321 and B.still_poison(b, holes=[(4300, 4400)], chunk=777) is None


def test_distortion_reference_plan_premises():
    """d_refRow of the large distortion call is a bijection that sends every row below the lines to a reference row above them and
    back; the reference rows ON the lines are each read by a crop row of another combination; the distinct (row, reference)
    combinations the referee has to answer are few."""
    n, row = B.ROWS_E31, CH * N * BS
    p = B.output_plan(n, row, 4, REAL)
    perm = B.ref_permutation(n)
    assert sorted(perm.tolist()) == list(range(n))
    low, high = REAL.L31 // (4 * row), REAL.E31 // row
    assert (perm[:low] > REAL.L32 // (4 * row)).all() and perm[:8].min() > n // 2 and (perm[high:] <= n // 2).all() and perm.max() == n - 1
    inv = np.argsort(perm)
    for line, (a, b) in p["on"].items():
        for r in (a, b):
            assert p["rowmap"][inv[r]] != p["rowmap"][r], f"reference row {r} on {line} is read by a row of its own combination"
    pairs, pairmap = B.distinct_pairs(p["rowmap"], perm)
    assert len(pairs) <= 2 * p["T"] and (pairs[:, 0] != pairs[:, 1]).all() and np.array_equal(pairs[pairmap][:, 0], p["rowmap"])


def test_clips_plan_premises():
    """32 776 clips of 32 768 samples: the input [n][2][nSamples] is 8 GiB + 2 MiB (every line), the corpus at a stride of 160 KiB is
    5 GiB (both byte lines, inside a file's stride), the planes [n][2][18][2048] are 9 GiB (every line); the rows on the lines and
    the first and last row are full-length clips, three table entries are short; the sizes the packing call is given put files
    beyond 2^32 bytes back to back."""
    import clips_testlib as ct
    n = B.ROWS_8G
    p = B.clips_plan(n, REAL)
    assert n * CH * B.CLIP_SAMPLES == REAL.E31 + (1 << 19) and p["n_blocks"] == ct.clip_blocks(BS, B.CLIP_SAMPLES) == 18
    assert [sorted(o) for o in p["on"]] == [["L31", "L32"], ["E31"], ["L31", "L32"], ["L31", "L32"], ["E31"]]
    a, b = p["on"][2]["L32"]
    assert a == b and a * B.CLIP_STRIDE < REAL.L32 < (a + 1) * B.CLIP_STRIDE
    on = sorted({r for lr in p["on"] for ab in lr.values() for r in ab} | {0, n - 1})
    assert (p["lengths"][p["rowmap"][on]] == B.CLIP_SAMPLES).all()
    assert sorted(p["lengths"][p["lengths"] < B.CLIP_SAMPLES].tolist()) == sorted(B.CLIP_SHORT) and (p["lengths"][p["rowmap"]] < B.CLIP_SAMPLES).sum() > 1000
    w = B.clip_waves(p["T"])
    assert len({x.tobytes() for x in w}) == p["T"] and w[2][:, 100:].any()
    sizes = B.ragged_sizes(n, B.CLIP_STRIDE).astype(np.int64)
    poffs = np.concatenate([[0], np.cumsum(sizes)])
    assert poffs[-1] > REAL.L32 + (100 << 20) and (sizes[1:] != sizes[:-1]).all() and sizes.min() > ct.ClipRef(BS, CH, w[0], ct.SCALAR).payload.size
    f = int(np.searchsorted(poffs, REAL.L32, "right")) - 1
    assert poffs[f] < REAL.L32 < poffs[f + 1], "a file lies across 2^32 bytes of the packed buffer"
