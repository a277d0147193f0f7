"""Plans and the checker of the address-line tests (tests/test_gpu_bigaddr_*.py, tests/test_bigaddr_capi.py): where files and
index rows lie so that a byte offset crosses 2^31 and 2^32 with a DIFFERENT valid file at every place a narrow offset would land,
which (file, first, count) every row of a multi-GiB output names so that two rows a line apart never agree, and the comparison of
a whole output with table[rowmap] in chunks.  The lines are parameters: the GPU tests run the plans at REAL, the CPU test runs the
same functions at TOY on numpy arrays and holds the checker against stores and loads whose offsets are formed narrowly (WRAPS).
Nothing here imports the library under test; torch is only ever met through the arrays a caller hands in."""
import collections
import functools
import numpy as np
from corpus_testlib import INDEX_DTYPE, PAD, Corpus, geom_files, oracle_file
from seek_testlib import ORACLE_CASES

Lines = collections.namedtuple("Lines", "L31 L32 E31")     # bytes, bytes, elements of the buffer's own type
REAL = Lines(1 << 31, 1 << 32, 1 << 31)
TOY = Lines(1 << 16, 1 << 17, 1 << 15)
STEREO = (2048, 2)


# ---------------------------------------------------------------------------------------------------------------------
# narrow offsets.  Every function is in the units of its line (bytes against L31 bytes, elements against E31, index entries
# against L31 / 8): `half` is the line a signed 32-bit value ends at, 2 * half the one an unsigned one ends at.
# ---------------------------------------------------------------------------------------------------------------------
def wrap_u32(x, half, size=None):
    """The offset truncated to 32 bits, unsigned.  (size: unused - the result is below x already; the three models share one signature.)"""
    return x % (2 * half)


def wrap_u31(x, half, size=None):
    """The offset truncated to 31 bits.  (size: unused, as in wrap_u32.)"""
    return x % half


def wrap_s32(x, half, size=None):
    """The offset truncated to 32 bits and sign-extended; with `size`, clamped into [0, size] as a model must be to stay in its buffer."""
    v = x % (2 * half)
    v = v - 2 * half if v >= half else v
    return v if size is None else max(0, min(v, size))


WRAPS = {"u32": wrap_u32, "u31": wrap_u31, "s32-clamped": wrap_s32}


def aliases(x, half):
    """Where a narrow form of offset x points instead: x mod 2^32, x mod 2^31 and x as a signed 32-bit value where that is >= 0,
    without x itself."""
    out = {wrap_u32(x, half), wrap_u31(x, half)}
    s = wrap_s32(x, half)
    if s >= 0:
        out.add(s)
    out.discard(x)
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------------
# placement: four live spans (below the first line, across it, across the second, wholly above it) and a decoy at every alias
# ---------------------------------------------------------------------------------------------------------------------
ROLES = ("low", "x31", "x32", "high")


def place(sizes, decoy_sizes, half, low, high_off, total):
    """sizes: the four live spans' lengths by role; decoy_sizes: lengths to draw decoys from, in order.  The span across the second
    line starts so that the line lies in its middle, the span across the first lies at that one's 31-bit alias (each is the other's
    decoy), `high` lies high_off above the second line.  -> {name: (start, length)} with decoys "decoy0", ... at every alias of a
    live start where no span starts yet.  Spans never overlap and end inside [0, total]."""
    at = {"low": low, "x32": 2 * half - sizes["x32"] // 2 - 1, "high": 2 * half + high_off}
    at["x31"] = at["x32"] - half
    spans = {r: (at[r], sizes[r]) for r in ROLES}
    pool = list(decoy_sizes)
    for r in ROLES:
        for a in aliases(at[r], half):
            if all(a != s for s, _ in spans.values()):
                spans[f"decoy{len(spans) - 4}"] = (a, pool.pop(0))
    check_placement(spans, half, total)
    return spans


def check_placement(spans, half, total):
    """The premises of a placement, as assertions: the roles lie where their names say, no two spans overlap, every alias of every
    span's start is the start of another span."""
    order = sorted(spans.values())
    assert order[0][0] >= 0 and order[-1][0] + order[-1][1] <= total, (order, total)
    assert all(a + n <= b for (a, n), (b, _) in zip(order, order[1:])), f"spans overlap: {order}"
    s, n = spans["low"];  assert s + n < half
    s, n = spans["x31"];  assert s < half < s + n
    s, n = spans["x32"];  assert half < s < 2 * half < s + n
    s, n = spans["high"]; assert s > 2 * half
    starts = {s: name for name, (s, _) in spans.items()}
    assert len(starts) == len(spans)
    for name, (s, _) in spans.items():
        for a in aliases(s, half):
            assert a in starts and starts[a] != name, f"{name} at {s}: no other span starts at its alias {a}"
    return True


# ---------------------------------------------------------------------------------------------------------------------
# files: the shared streams of a geometry and as many further oracle-encoded ones as a plan needs, no two alike
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def distinct_files(geom, n, short_blocks=12):
    """n Files of one geometry: the shared streams (seek_testlib / corpus_testlib), one more file of the shared length and short ones
    behind it, every payload different from every other."""
    geom = tuple(geom)
    bs, ch, q, sid = next(c for c in ORACLE_CASES if (c[0], c[1]) == geom)
    out = list(geom_files(geom)) + [oracle_file(bs, ch, q, sid + 17)]
    extra = 0
    while len(out) < n:
        out.append(oracle_file(bs, ch, q, sid + 20 + extra, 11, short_blocks))
        extra += 1
    out = out[:n]
    assert len({f.payload.tobytes() for f in out}) == n, "two files are alike"
    assert all((f.bits > 0).all() for f in out)
    return out


class RaggedBig:
    """A ragged corpus whose payloads and index rows lie across the lines.  files: Files in file-number order 0 .. G - 1;
    pay / idx: for each, its (start, length) in the payload buffer (bytes) and in the index (entries, length K + 1).  Real file g is
    file 2 g of the tables; file 2 g + 1 is the bytes between g and g + 1.  The payloads lie in DESCENDING order of file number,
    so every in-between file has falling payload offsets: no call looks at one byte or entry of it.
    -> poffs / ioffs int64 [2 G], blocks int32 [2 G - 1], pieces of the two buffers as [(offset, array)];
    every index row has `cap` entries, {-1, 0} behind a file's closing one."""

    def __init__(self, files, pay, idx, pay_total, idx_total, cap):
        G = len(files)
        assert all(pay[g][1] == files[g].payload.size and idx[g][1] == cap > files[g].K for g in range(G))
        assert all(pay[g + 1][0] + pay[g + 1][1] <= pay[g][0] for g in range(G - 1)), "payloads descend with the file number"
        assert all(idx[g][0] + idx[g][1] <= idx[g + 1][0] for g in range(G - 1)), "index rows ascend with the file number"
        assert pay[0][0] + pay[0][1] + PAD <= pay_total and idx[-1][0] + idx[-1][1] <= idx_total
        self.files, self.G, self.F = list(files), G, 2 * G - 1
        self.pay_total, self.idx_total = pay_total, idx_total
        self.poffs = np.array([v for s, n in pay for v in (s, s + n)], np.int64)
        self.ioffs = np.array([v for s, n in idx for v in (s, s + n)], np.int64)
        self.blocks = np.zeros(self.F, np.int32)
        self.blocks[0::2] = [f.K for f in files]
        self.pay_pieces = [(pay[g][0], files[g].payload) for g in range(G)]
        self.idx_pieces = [(idx[g][0], files[g].row(cap)) for g in range(G)]
        self.cap = cap
        assert all(self.poffs[f + 1] < self.poffs[f] for f in range(1, self.F, 2)), "an in-between file could be walked"
        self.model = Corpus(files)                          # the same files in a plain corpus: file g there is file 2 g here

    def number(self, g):
        return 2 * g


def ragged_big(geom, lines, pay_slack, idx_slack_bytes):
    """The ragged layout of the address tests for one geometry: a payload buffer of L32 + pay_slack bytes and an index of L32 +
    idx_slack_bytes bytes, the four roles and the decoys in each.  Every index row has the longest file's K + 1 entries, so any row
    fits any span: the payloads descend with the file number, the rows ascend.  -> (RaggedBig, payload spans, index spans) by name."""
    files = distinct_files(geom, 6)
    kmax = max(f.K for f in files)
    long_ = sorted([f for f in files if f.K == kmax], key=lambda f: f.payload.size)
    rest = [f for f in files if f.K != kmax] + long_[2:]
    role_file = {"x32": long_[0], "x31": long_[1], "low": rest[0], "high": rest[1]}
    pay_total = lines.L32 + pay_slack
    pspans = place({r: role_file[r].payload.size for r in ROLES}, [f.payload.size for f in rest[2:]], lines.L31, 1001,
                   pay_slack // 2 + 37, pay_total - PAD)
    named = dict(role_file)
    named.update({f"decoy{i}": f for i, f in enumerate(rest[2:]) if f"decoy{i}" in pspans})
    order = sorted(named, key=lambda name: -pspans[name][0])           # file numbers: payloads descending
    cap = kmax + 1
    idx_total = (lines.L32 + idx_slack_bytes) // 8
    ispans = place({r: cap for r in ROLES}, [cap] * 4, lines.L31 // 8, 3, idx_slack_bytes // 16 + 5, idx_total)
    assert len(ispans) == len(order), "as many index spans as files"
    rows = sorted(ispans.items(), key=lambda kv: kv[1][0])             # ... index rows ascending
    rb = RaggedBig([named[name] for name in order], [pspans[name] for name in order], [sp for _, sp in rows], pay_total, idx_total, cap)
    return rb, {name: pspans[name] for name in order}, {f"{irole} (file {order[g]})": sp for g, (irole, sp) in enumerate(rows)}


# ---------------------------------------------------------------------------------------------------------------------
# the strided layouts: which file numbers are live and which lie at their aliases
# ---------------------------------------------------------------------------------------------------------------------
MANY_STRIDE_LOG2 = 20
MANY_FILES = 4100
MANY_LIVE = (0, 2047, 2048, 4095, 4096, 4099)
MANY_DECOYS = (1999, 2000, 2051, 3)


def strided_many(geom, lines, stride, n_files, live, decoys):
    """A strided corpus of n_files files `stride` bytes apart in which only `live` and `decoys` hold a file (all different) and every
    other file has 0 bytes and 0 blocks.  -> dict(files {number: File}, nbytes int32 [n_files], blocks int32 [n_files], istride,
    index [n_files][istride] of INDEX_DTYPE).  Asserted: live files lie below, at and above both lines, and every alias of a live
    file's byte offset that is a file's start is the start of a file that holds another stream."""
    numbers = list(live) + list(decoys)
    fs = distinct_files(geom, len(numbers))
    files = dict(zip(numbers, fs))
    assert all(f.payload.size + PAD <= stride for f in fs)
    starts = {n * stride: n for n in numbers}
    assert any(n * stride < lines.L31 for n in live) and any(n * stride == lines.L31 for n in live) and any(n * stride >= lines.L32 for n in live)
    hit = 0
    for n in live:
        for a in aliases(n * stride, lines.L31):
            assert a % stride == 0 and a in starts and starts[a] != n, f"file {n}: its alias {a} is no other file's start"
            hit += 1
    assert hit >= 4, "files at 2^31, below 2^32, at 2^32 and above it each have an alias"
    istride = max(f.K for f in fs) + 1
    nbytes, blocks = np.zeros(n_files, np.int32), np.zeros(n_files, np.int32)
    index = np.zeros((n_files, istride), INDEX_DTYPE)
    index["ByteOffs"][:, 1:] = -1
    for n, f in files.items():
        nbytes[n], blocks[n], index[n] = f.payload.size, f.K, f.row(istride)
    return dict(files=files, nbytes=nbytes, blocks=blocks, istride=istride, index=index, stride=stride, n_files=n_files)


def strided_huge(geom, lines, extra=4096):
    """Three files L31 + extra bytes apart: file 1 starts across the first line from file 0, file 2 above the second.  Their aliases
    (extra and 2 * extra) lie inside file 0's stride, behind file 0's own bytes: a decoy stream is written at each.  A strided index
    is addressed by file number, so these decoys have NO index row of their own: a narrow payload offset would walk file 1's or
    file 2's ByteOffs over the decoy's bytes - wrong output from bytes inside the buffer, not another file's valid decode.
    -> strided_many()'s dict with decoy_at {byte offset: File}."""
    stride = lines.L31 + extra
    fs = distinct_files(geom, 6)
    small = sorted(fs, key=lambda f: f.payload.size)
    f0 = next(f for f in small if f.payload.size + PAD <= extra)       # file 0 ends in front of the first decoy
    others = [f for f in fs if f is not f0]
    d1 = next(f for f in sorted(others, key=lambda f: f.payload.size) if f.payload.size <= extra)
    others = [f for f in others if f is not d1]
    files = {0: f0, 1: others[0], 2: others[1]}
    decoy_at = {extra: d1, 2 * extra: others[2]}
    assert aliases(stride, lines.L31) == [extra] and set(aliases(2 * stride, lines.L31)) == {2 * extra}
    assert stride < lines.L32 < 2 * stride and 2 * extra + others[2].payload.size < stride
    istride = max(f.K for f in fs) + 1
    nbytes, blocks = np.zeros(3, np.int32), np.zeros(3, np.int32)
    index = np.zeros((3, istride), INDEX_DTYPE)
    for n, f in files.items():
        nbytes[n], blocks[n], index[n] = f.payload.size, f.K, f.row(istride)
    return dict(files=files, nbytes=nbytes, blocks=blocks, istride=istride, index=index, stride=stride, n_files=3, decoy_at=decoy_at)


# ---------------------------------------------------------------------------------------------------------------------
# the row plan of a large output: row i names combos[rowmap[i]]
# ---------------------------------------------------------------------------------------------------------------------
def combos_of(files, n_blocks, n_short=6):
    """(file, first, count) over Files `files`: every start that leaves a full row of n_blocks live blocks, then a few short rows
    (count below n_blocks: the rest of the row is zero fill).  -> (combos, number of full ones)."""
    full = [(f, k, n_blocks) for k in range(0, 64) for f in range(len(files)) if k + n_blocks <= files[f].K]
    short = [(i % len(files), i, (3 * i + 1) % n_blocks) for i in range(n_short)]
    return full + short, len(full)


def _is_prime(p):
    return p > 1 and all(p % q for q in range(2, int(p ** 0.5) + 1))


def line_rows(n, row_units, lines_units):
    """For a buffer of n rows of row_units units each: {line: (first row that touches it, last row that touches it)} for the lines
    (in the same units) that lie inside the buffer."""
    out = {}
    for name, L in lines_units.items():
        if 0 < L < n * row_units:
            out[name] = ((L - 1) // row_units, L // row_units)
    return out


def row_plan(n, combos, n_full, dists, full_rows):
    """rowmap int64 [n]: row i names combos[(i + shift) mod T], T the largest prime <= len(combos) that divides no distance of
    `dists` (rows that far apart then name different combinations, as do neighbours), shift the smallest that gives every row of
    full_rows a full combination."""
    dists = sorted({int(d) for d in dists if 0 < int(d) < n} | {1})
    T = next(t for t in range(len(combos), 1, -1) if _is_prime(t) and all(d % t for d in dists))
    full_at = np.array([j < n_full for j in range(T)])
    assert T > n_full >= T // 2, "the table holds short rows, and mostly full ones"
    shift = next(s for s in range(T) if all(full_at[(i + s) % T] for i in full_rows))
    rowmap = (np.arange(n, dtype=np.int64) + shift) % T
    for d in dists:
        assert (rowmap[d:] != rowmap[:-d]).all(), d
    assert (rowmap[list(full_rows)] < n_full).all()
    assert (rowmap >= n_full).any(), "no short row in the plan"
    return rowmap, T


def plan_rows(n, combos, n_full, spans):
    """row_plan() for an output whose row measures row_units units against the lines {name: L} of those units, for each pair in
    `spans` = [(row_units, {name: L})]: bytes and elements of the same buffer.  -> (rowmap, T, {line name: (first, last) row on it})."""
    dists, on = [], {}
    for row_units, ls in spans:
        for name, (a, b) in line_rows(n, row_units, ls).items():
            on[name] = (a, b)
            L = ls[name]
            dists += [L // row_units, -(-L // row_units)]
    full_rows = sorted({0, n - 1} | {r for ab in on.values() for r in ab})
    rowmap, T = row_plan(n, combos, n_full, dists, full_rows)
    return rowmap, T, on


# ---------------------------------------------------------------------------------------------------------------------
# poison and the checker: numpy arrays here and on the CPU, torch tensors on the device - the same text
# ---------------------------------------------------------------------------------------------------------------------
def _xp(a):
    if isinstance(a, np.ndarray):
        return np, {}
    import torch
    return torch, {"device": a.device}


def poison_words(xp, kw, a, b):
    """int32 words a .. b - 1 of the pattern: position-dependent, never 0."""
    i = xp.arange(a, b, dtype=xp.int64, **kw)
    v = ((i * 0x9E3779B1) ^ (i >> 13)) & 0x3FFFFFFF | 0x40000000
    return v.astype(np.int32) if xp is np else v.to(xp.int32)


def poison(words, chunk=1 << 26):
    """Fill a flat int32 view with the pattern, in chunks."""
    xp, kw = _xp(words)
    for a in range(0, words.shape[0], chunk):
        b = min(words.shape[0], a + chunk)
        words[a:b] = poison_words(xp, kw, a, b)


def still_poison(words, holes=(), chunk=1 << 26):
    """The first word of a flat int32 view that no longer holds the pattern, outside the word ranges `holes` = [(a, b)]; None if all do."""
    xp, kw = _xp(words)
    for a in range(0, words.shape[0], chunk):
        b = min(words.shape[0], a + chunk)
        ne = words[a:b] != poison_words(xp, kw, a, b)
        for ha, hb in holes:
            if ha < b and hb > a:
                ne[max(ha, a) - a:min(hb, b) - a] = False
        if bool(ne.any()):
            return a + _first_true(ne)
    return None


def _first_true(flat):
    nz = flat.reshape(-1).nonzero()
    return int(nz[0][0]) if isinstance(nz, tuple) else int(nz[0, 0])


def first_diff(out, table, rowmap, chunk=512):
    """out [n][row] against table[rowmap] ([T][row], the same integer type; rowmap int64 [n], with `out`), every element, in chunks of
    rows.  -> None, or (row, element of the row) of the first difference."""
    n = out.shape[0]
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        ne = out[a:b] != table[rowmap[a:b]]
        if bool(ne.any()):
            at = _first_true(ne)
            return a + at // out.shape[1], at % out.shape[1]
    return None


def name_diff(diff, shape, rowmap, combos):
    """A message for first_diff()'s result: the row, what it names, and the element as an index of a row of `shape`."""
    if diff is None:
        return "equal"
    row, el = diff
    return f"row {row} (file, first, count) = {combos[int(rowmap[row])]}: first difference at {tuple(int(v) for v in np.unravel_index(el, shape))} of {shape}"


# ---------------------------------------------------------------------------------------------------------------------
# expected rows of the families, per combination, from the oracle (corpus_testlib)
# ---------------------------------------------------------------------------------------------------------------------
def pcm_table(files, combos, n_blocks):
    """float32 [T][n_blocks * bs * ch] and int32 [T][n_blocks]: File.expected_pcm of every combination."""
    rows = [files[f].expected_pcm(k, n_blocks, c) for f, k, c in combos]
    return np.stack([r[0].reshape(-1) for r in rows]), np.stack([r[1] for r in rows])


def spec_table(files, combos, n_blocks, lr=False):
    """float32 [T][ch * n_blocks * bs], wc int32 [T][n_blocks], bits int32 [T][n_blocks]: File.expected_spec of every combination."""
    rows = [files[f].expected_spec(k, n_blocks, c, lr) for f, k, c in combos]
    return np.stack([r[0].reshape(-1) for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])


def sample_row(f, start, n_samples, length=None):
    """Row (start[, length]) of a sample-crop call on File f -> (float32 [ch][n_samples], the sizes of the blocks it touches as a
    list from block start // bs on): the oracle's decoded stream sliced at the sample, zeros behind the length and the file's end."""
    bs, ch = f.bs, f.ch
    out = np.zeros((ch, n_samples), np.float32)
    ln = n_samples if length is None else max(0, min(n_samples, int(length)))
    bits = []
    if start >= 0 and start // bs <= f.K and ln > 0:
        stream = f.pcm.reshape(f.K * bs, ch).T
        end = min(start + ln, f.K * bs)
        if end > start:
            out[:, :end - start] = stream[:, start:end]
        bits = [int(f.obits[b]) if b < f.K else 0 for b in range(start // bs, (start + ln - 1) // bs + 1)]
    return out, bits


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_bigaddr_rows.py, planned here so that tests/test_bigaddr_capi.py asserts their premises without a GPU
# ---------------------------------------------------------------------------------------------------------------------
ROW_BLOCKS = 16                                            # blocks per row of the large outputs
ROWS_4G, ROWS_8G = 16392, 32776                            # float rows of 256 KiB: 4 GiB + 2 MiB and 8 GiB + 2 MiB
ROWS_E31 = 34961                                           # rows of [2][15 x 2048 (+ 1)] floats: 8 more than reach element 2^31 (8 GiB + 2 MiB)


@functools.lru_cache(maxsize=None)
def rows_files():
    """The files the large outputs are cut from: the stereo 2048 streams long enough for a full row of ROW_BLOCKS blocks."""
    return [f for f in distinct_files(STEREO, 4) if f.K >= ROW_BLOCKS + 8]


def output_plan(n, row_elems, esize, lines, n_blocks=ROW_BLOCKS):
    """The row plan of an output of n rows of row_elems elements of esize bytes: the byte lines and the element line that lie inside
    it.  -> dict(rowmap, T, on {line: (first, last) row on it}, combos, n_full)."""
    combos, n_full = combos_of(rows_files(), n_blocks)
    rowmap, T, on = plan_rows(n, combos, n_full, [(row_elems * esize, {"L31": lines.L31, "L32": lines.L32}), (row_elems, {"E31": lines.E31})])
    return dict(rowmap=rowmap, T=T, on=on, combos=combos[:T], n_full=n_full, n=n)


def rows_corpus():
    """The small strided corpus the large outputs read: corpus_testlib.Corpus of rows_files()."""
    return Corpus(rows_files())


SAMPLE_ROW = (ROW_BLOCKS - 1) * 2048 + 1                   # samples per row of the large sample-crop output: 16 blocks at the worst start


def sample_combos(files, n_samples, n_short=6):
    """(file, start sample, length) over Files `files`: starts at every alignment inside a block that leave n_samples live samples,
    then a few short rows (zeros behind the length).  -> (combos, number of full ones)."""
    full = []
    for k in range(0, 64):
        for f in range(len(files)):
            start = k * files[f].bs + (389 * (k + 3 * f) + 1) % files[f].bs
            if start + n_samples <= files[f].K * files[f].bs:
                full.append((f, start, n_samples))
    short = [(i % len(files), 1000 * i + 7, (n_samples * (i + 1)) // 9) for i in range(n_short)]
    return full + short, len(full)


def sample_plan(n, n_samples, ch, esize, lines):
    """output_plan() for a sample-crop output [n][ch][n_samples] of elements of esize bytes."""
    combos, n_full = sample_combos(rows_files(), n_samples)
    row = ch * n_samples
    rowmap, T, on = plan_rows(n, combos, n_full, [(row * esize, {"L31": lines.L31, "L32": lines.L32}), (row, {"E31": lines.E31})])
    return dict(rowmap=rowmap, T=T, on=on, combos=combos[:T], n_full=n_full, n=n)


def sample_table(files, combos, n_samples, n_bits):
    """float32 [T][ch * n_samples] and int32 [T][n_bits]: sample_row() of every combination."""
    rows = [sample_row(files[f], s, n_samples, ln) for f, s, ln in combos]
    bits = np.zeros((len(rows), n_bits), np.int32)
    for i, (_, b) in enumerate(rows):
        bits[i, :len(b)] = b
    return np.stack([r[0].reshape(-1) for r in rows]), bits


def stream_plan(n, spans, t_max=31):
    """The row plan of the streaming calls: stream i carries table entry i mod T, T the largest prime <= t_max that divides no
    distance at which a line of `spans` = [(row units, {line: L})] falls (floor and ceiling), so streams a line apart differ in
    every buffer of the call, as neighbours do.  -> (rowmap int64 [n], T, {line: (first, last) row on it} per span)"""
    dists, on = {1}, []
    for row_units, ls in spans:
        lr = line_rows(n, row_units, ls)
        on.append(lr)
        for name in lr:
            dists |= {ls[name] // row_units, -(-ls[name] // row_units)}
    T = next(t for t in range(t_max, 1, -1) if _is_prime(t) and all(d % t for d in dists))
    rowmap = np.arange(n, dtype=np.int64) % T
    for d in dists:
        assert (rowmap[d:] != rowmap[:-d]).all(), d
    return rowmap, T, on


def ref_permutation(n):
    """d_refRow of the large distortion call: crop row i is held against reference row (i + n // 2 + 1) mod n - a bijection that
    sends the low rows to the high reference rows and the high rows back to the low ones.  -> int64 [n]"""
    return (np.arange(n, dtype=np.int64) + n // 2 + 1) % n


def distinct_pairs(rowmap, perm):
    """The distinct (combination of the crop row, combination of its reference row) pairs of a plan under d_refRow = perm
    -> (pairs int64 [P][2], pairmap int64 [n]: row i is pairs[pairmap[i]])"""
    both = np.stack([rowmap, rowmap[perm]], axis=1)
    pairs, pairmap = np.unique(both, axis=0, return_inverse=True)
    return pairs, pairmap.reshape(-1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the clips calls at 32 776 rows: clips of 16 blocks (32 768 samples), so that the input [n][2][nSamples] is 8 GiB + 2 MiB
# ---------------------------------------------------------------------------------------------------------------------
CLIP_SAMPLES = ROW_BLOCKS * 2048
CLIP_STRIDE = 160 << 10                                    # payloadStride of the corpus the clips calls write: 32 776 files are 5 GiB
CLIP_SHORT = (1, 5 * 2048 + 7, 0)                          # d_len of the three short table entries (one block, some, an empty row)


def clips_plan(n, lines, bs=2048, ch=2, t_max=31):
    """The rows of the large clips calls: row i is table entry i mod T (stream_plan over the input rows in bytes and elements, the
    corpus rows in bytes and the spectra planes in bytes and elements); three entries that no row on a line, nor the first or the
    last row, names are short (CLIP_SHORT).  -> dict(rowmap, T, on, lengths int32 [T], n_blocks: planes per row)"""
    nb = CLIP_SAMPLES // bs + 2
    b = {"L31": lines.L31, "L32": lines.L32}
    spans = [(ch * CLIP_SAMPLES * 4, b), (ch * CLIP_SAMPLES, {"E31": lines.E31}), (CLIP_STRIDE, b), (ch * nb * bs * 4, b), (ch * nb * bs, {"E31": lines.E31})]
    rowmap, T, on = stream_plan(n, spans, t_max)
    held = {int(rowmap[r]) for lr in on for ab in lr.values() for r in ab} | {int(rowmap[0]), int(rowmap[n - 1])}
    free = [t for t in range(T) if t not in held]
    assert len(free) >= len(CLIP_SHORT), "no table entry left for the short rows"
    lengths = np.full(T, CLIP_SAMPLES, np.int32)
    lengths[free[:len(CLIP_SHORT)]] = CLIP_SHORT
    return dict(rowmap=rowmap, T=T, on=on, lengths=lengths, n_blocks=nb, n=n)


@functools.lru_cache(maxsize=None)
def clip_waves(T, bs=2048, ch=2):
    """float32 [T][ch][CLIP_SAMPLES] on the PCM16 grid, every clip different; samples behind a row's length are not zero."""
    from ulc_testlib import synth_pcm
    return np.stack([np.ascontiguousarray(synth_pcm(200 + t, CLIP_SAMPLES, ch, 44100, transient=True, seed=17).T) for t in range(T)])


def ragged_sizes(n, stride):
    """The d_payloadBytes the large ulcx_corpus_ragged_dev call is given: 128 KiB and up to 8 KiB more per file, no two
    neighbours alike - 32 776 files are more than 2^32 bytes back to back.  -> int32 [n]"""
    out = ((128 << 10) + (np.arange(n, dtype=np.int64) * 37) % 8191).astype(np.int32)
    assert out.max() <= stride
    return out
