"""Inputs and oracle references of the clip tests (tests/test_clips_capi.py, tests/test_gpu_clips.py,
tests/test_gpu_clips_paths.py): channels-first clips of different length, what the oracle's encoder writes for each clip alone
(oracle_encode_debug of the interleaved clip zero-padded to the tool's block count), the index of that payload from the oracle's
decoder (seek_testlib.oracle_walk), the numpy restatement of ulcx_corpus_ragged_dev's offsets and capacity rule, and the synthetic
strided corpora the ragged call is run on.  CPU only."""
import collections
import functools
import numpy as np
from ulc_testlib import synth_pcm, oracle_encode_debug, oracle_decode_stream
from seek_testlib import oracle_walk, SEED0
from corpus_testlib import INDEX_DTYPE
from rates_testlib import mode_of

RATE = 44100
GEOMS = [(256, 2), (512, 1), (256, 3)]                      # the stereo vector path, mono, the generic channel loop
SCALAR = (-50.0, 0.0)                                       # VBR 50 in the tool's convention
TABLE = [(-50.0, 0.0), (64.0, 0.0), (96.0, 1.5), (-30.0, 0.0), (48.0, 0.0), (80.0, 2.0), (-70.0, 0.0)]     # VBR, CBR and ABR rows mixed
# The seven (clip, length) pairs of a test: nSamples of the call and the rows' lengths.  Row i of a call of more rows is pair i % 7.
Case = collections.namedtuple("Case", "T lengths")


def clip_blocks(bs, n):
    """The tool's block count for a file of n samples (tools/ulcEncodeTool.c:93-98); 0 for an empty clip."""
    return (n + bs - 1) // bs + 2 if n >= 1 else 0


def n_samples(bs):
    return 5 * bs + 3                                       # odd: the planes of rows and channels start at every alignment


def lengths(bs):
    return [0, 1, bs - 1, bs, bs + 1, 3 * bs + 7, n_samples(bs)]


def short_case(bs):
    """tests/test_gpu_clips.py: 8 blocks at the most, four chunks of maxBlocksPerCall = 2."""
    return Case(n_samples(bs), tuple(lengths(bs)))


# tests/test_gpu_clips_paths.py, part A: (BlockSize, nChan, nStreams of the object, maxBlocksPerCall).  23 blocks: chunks of
# 8 + 8 + 7 blocks (pipelined in 4, 4, 3 transform chunks) or of 6 + 6 + 6 + 5 (3, 3, 3, then no pipeline); with
# maxBlocksPerCall = 2 eleven chunks and a single block.
PATH_GEOMS = [(2048, 2, 70, 8), (4096, 2, 8, 8), (2048, 1, 8, 6), (16384, 1, 4, 2)]
PATH_BLOCKS = [0, 3, 8, 9, 16, 17, 23]
PATH_ROWS = {(16384, 1): (0, 1, 3, 6)}                     # the pairs a geometry runs (default: all seven); the oracle is the cost


def path_case(bs):
    """A row's last block at every position relative to a chunk of 8: no block, inside the first chunk, the first chunk's last
    block, the second chunk's first, and the same one chunk on; the longest row ends in the short last chunk."""
    T = 20 * bs + 3
    return Case(T, (0, 1, 6 * bs, 6 * bs + 1, 14 * bs, 14 * bs + 1, T))


def path_rows(bs, ch):
    return PATH_ROWS.get((bs, ch), tuple(range(7)))


def path_cut_strides(refs):
    """Part A's two capacities that stop the longest row inside the second chunk of 8: a payloadStride one byte short of row 6's
    eleventh block, and indexStride - 1 = 9 blocks."""
    return int(refs[6].sizes[:11].sum()) - 1, 10


def grid_case(bs):
    """tests/test_gpu_clips_paths.py, part B: more rows than the row kernels' grid, 5 blocks at the most."""
    T = 2 * bs + 1
    return Case(T, (0, 1, bs - 1, bs, bs + 1, 2 * bs, T))


GRID_GEOM = (256, 1, 16384 + 5, 2)                          # as PATH_GEOMS; the call has as many rows as the object streams


@functools.lru_cache(maxsize=None)
def wave(bs, ch, T=None):
    """[7][ch][T] float32 on the PCM16 grid (T: n_samples(bs) by default): synth_pcm per row, transposed.  Samples behind a
    row's length are NOT zero: the call must not read them into the clip."""
    T = n_samples(bs) if T is None else T
    return np.stack([np.ascontiguousarray(synth_pcm(20 + i, T, ch, RATE, transient=True, seed=17).T) for i in range(7)])


class ClipRef:
    """One clip under one setting, from the oracle alone: blocks, sizes, payload, index row."""

    def __init__(self, bs, ch, clip, setting):
        L = clip.shape[1]
        self.bs, self.ch, self.L, self.nb = bs, ch, L, clip_blocks(bs, L)
        self.slot = 2 * ch * bs + 16
        if self.nb == 0:
            self.blocks, self.bits, self.wc = np.zeros((0, self.slot), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32)
        else:
            pcm = np.zeros((self.nb * bs, ch), np.float32)
            pcm[:L] = clip.T
            mode, p0, p1 = mode_of(setting)
            r = oracle_encode_debug(pcm, bs, RATE, mode, p0, p1, slot=self.slot)
            self.blocks, self.bits, self.wc = r["out"], r["bits"], r["wc"]
            assert (self.bits > 0).all() and (self.bits % 8 == 0).all()
        self.sizes = self.bits.astype(np.int64) // 8
        self.payload = (np.concatenate([self.blocks[k, :self.sizes[k]] for k in range(self.nb)]) if self.nb else np.zeros(0, np.uint8)).astype(np.uint8)
        self._rows = {}

    def kept(self, payload_stride, index_stride):
        """Leading whole blocks that fit the two capacities."""
        m, off = 0, 0
        while m < self.nb and m + 1 <= index_stride - 1 and off + self.sizes[m] <= payload_stride:
            off += int(self.sizes[m]); m += 1
        return m

    def index_row(self, index_stride, blocks=None):
        """What ulcx_index_packed_rows_dev builds from the payload's first `blocks` blocks with maxBlocks = index_stride - 1: the
        oracle decoder's walk of those bytes (offsets, generator states), {-1, 0} behind the closing entry."""
        m = self.nb if blocks is None else blocks
        if (index_stride, m) in self._rows:                 # (a reference is shared by the rows and tests that use it)
            return self._rows[index_stride, m].copy()
        nbytes = int(self.sizes[:m].sum())
        row = np.zeros(index_stride, INDEX_DTYPE)
        row["ByteOffs"] = -1
        row["ByteOffs"][0], row["RngState"][0] = 0, SEED0
        if m:
            wbits, offs, seeds, inside = oracle_walk(self.payload, nbytes, self.ch, self.bs, index_stride - 1)
            assert inside and len(wbits) == m and np.array_equal((wbits + 7) // 8, self.sizes[:m])      # the oracle's decoder reads back the oracle's encoder
            row["ByteOffs"][:m + 1], row["RngState"][:m + 1] = offs, seeds
        self._rows[index_stride, m] = row
        return row.copy()

    def decoded(self):
        """[nb * bs][ch]: the oracle's sequential decode of the blocks."""
        rc, pcm, _ = oracle_decode_stream(self.blocks, self.ch, self.bs)
        assert rc == 0
        return pcm


@functools.lru_cache(maxsize=None)
def row_ref(bs, ch, i, table=False, case=None):
    """Pair i's reference under the scalar setting or its row of the mixed table.  (PCM16 input has the float input's reference:
    the waves are on the PCM16 grid.)"""
    case = case or short_case(bs)
    return ClipRef(bs, ch, wave(bs, ch, case.T)[i][:, :case.lengths[i]], TABLE[i] if table else SCALAR)


def refs(bs, ch, table=False, pcm16=False, case=None, rows=None):
    """The references of the call rows `rows` (pair numbers; default: the seven pairs in order)."""
    return [row_ref(bs, ch, i % 7, table, case) for i in (range(7) if rows is None else rows)]


def ragged_plan(payload_bytes, payload_stride, index_blocks, index_stride, payload_cap, index_cap):
    """ulcx_corpus_ragged_dev's tables restated: file f has clamp(bytes, 0, stride) bytes and clamp(blocks, 0, index_stride - 1) + 1
    entries; the files are laid out in order while both running totals stay within the capacities; the first that does not fit and
    all behind it get an empty range and 0 blocks.  -> (payload_offs [F + 1], index_offs [F + 1], out_blocks [F], need [2])."""
    b = np.clip(np.asarray(payload_bytes, np.int64), 0, payload_stride)
    k = np.clip(np.asarray(index_blocks, np.int64), 0, index_stride - 1)
    F = b.size
    poffs, ioffs, blocks = np.zeros(F + 1, np.int64), np.zeros(F + 1, np.int64), np.zeros(F, np.int32)
    open_ = True
    for f in range(F):
        open_ = open_ and poffs[f] + b[f] <= payload_cap and ioffs[f] + k[f] + 1 <= index_cap
        poffs[f + 1] = poffs[f] + (b[f] if open_ else 0)
        ioffs[f + 1] = ioffs[f] + (k[f] + 1 if open_ else 0)
        blocks[f] = k[f] if open_ else 0
    return poffs, ioffs, blocks, np.array([b.sum(), (k + 1).sum()], np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Synthetic strided corpora for ulcx_corpus_ragged_* (tests/test_gpu_clips_paths.py, part C): no codec is involved, so the
# payload is random bytes and an index entry is two arbitrary words.
# ---------------------------------------------------------------------------------------------------------------------
RAGGED_ISTRIDE = 4
Corpus = collections.namedtuple("Corpus", "pay nbytes index blocks")       # uint8 [F][stride], int32 [F], INDEX_DTYPE [F][4], int32 [F]
NO_CAP = 1 << 40


def _corpus(rng, nbytes, blocks, stride):
    F = len(nbytes)
    index = rng.integers(0, 1 << 32, (F, RAGGED_ISTRIDE, 2), dtype=np.uint64).astype(np.uint32).view(INDEX_DTYPE).reshape(F, RAGGED_ISTRIDE)
    return Corpus(rng.integers(0, 256, (F, stride), dtype=np.uint8), np.asarray(nbytes, np.int32), index, np.asarray(blocks, np.int32))


def plan_of(c, pcap=NO_CAP, icap=NO_CAP):
    return ragged_plan(c.nbytes, c.pay.shape[1], c.blocks, c.index.shape[1], pcap, icap)


def cut_file(c, pcap, icap):
    """The first file the capacities leave out (a file that is laid out has at least its closing entry); F when all fit."""
    laid = np.diff(plan_of(c, pcap, icap)[1]) > 0
    return int(np.argmin(laid)) if not laid.all() else laid.size


TILE_FILES = (1, 255, 256, 257, 513, 1000)                 # k_corpus_offsets walks the table in tiles of 256 files
TILE_STRIDE = 37                                           # odd: the files start at every alignment
TILE_MARKS = (0, 256, 300, 400, 450, 512, 700)             # files of at least one byte: a capacity a byte short of one cuts there


@functools.lru_cache(maxsize=None)
def corpus_tiles(F):
    rng = np.random.default_rng([41, F])
    nbytes = rng.integers(0, TILE_STRIDE + 1, F)
    for f in TILE_MARKS:
        if f < F:
            nbytes[f] = max(1, nbytes[f])
    return _corpus(rng, nbytes, rng.integers(0, RAGGED_ISTRIDE, F), TILE_STRIDE)


def tile_caps(F):
    """[(what, payloadCap, indexCap, first file left out)] for the corpus of F files.  513 files: the six cases of the second
    and third tile (the third tile of 513 files is file 512 alone); 1000 files: a cut further inside the third tile."""
    c = corpus_tiles(F)
    poffs, ioffs, _, need = plan_of(c)
    b = np.clip(c.nbytes.astype(np.int64), 0, TILE_STRIDE)
    short = lambda f: int(poffs[f] + b[f] - 1)             # a byte short of file f
    caps = [("everything fits exactly", int(need[0]), int(need[1]), F), ("room to spare", int(need[0]) + 5, int(need[1]) + 3, F)]
    if F == 513:
        caps += [("cut at exactly 256 files", short(256), int(need[1]), 256), ("cut inside the second tile", short(400), int(need[1]), 400),
                 ("cut inside the third tile", short(512), int(need[1]), 512), ("the first file does not fit", short(0), int(need[1]), 0),
                 ("the index cuts before the payload", short(450), int(ioffs[301]) - 1, 300)]
    if F == 1000:
        caps += [("cut inside the third tile, above file 512", short(700), int(need[1]), 700)]
    return caps


UNTRUSTED_BYTES = {3: -1, 100: -2 ** 31, 200: TILE_STRIDE + 1, 17: 2 ** 31 - 1, 259: 2 ** 31 - 1, 255: -1, 256: TILE_STRIDE + 1}
UNTRUSTED_BLOCKS = {5: -1, 150: RAGGED_ISTRIDE, 270: 2 ** 31 - 1, 259: -1, 255: 2 ** 31 - 1, 17: RAGGED_ISTRIDE}


@functools.lru_cache(maxsize=None)
def corpus_untrusted():
    """300 files whose two count tables hold values no encode call writes: the call clamps them (ragged_plan)."""
    rng = np.random.default_rng(43)
    nbytes, blocks = rng.integers(0, TILE_STRIDE + 1, 300), rng.integers(0, RAGGED_ISTRIDE, 300)
    for f, v in UNTRUSTED_BYTES.items():
        nbytes[f] = v
    for f, v in UNTRUSTED_BLOCKS.items():
        blocks[f] = v
    return _corpus(rng, nbytes, blocks, TILE_STRIDE)


COPY_STRIDE = 2053                                         # = 1 mod 4: file f starts at (f & 3) behind the corpus's base
COPY_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9)
COPY_BIG = {21: 4 * 256 * 2 + 3, 42: 4 * 256 + 1}          # the word loop's second trip (and head and tail bytes); its exact end
COPY_SEED = 14                                             # (the first seed whose table covers what tests/test_clips_capi.py asks of it)


@functools.lru_cache(maxsize=None)
def corpus_bytecopy():
    """64 files for wg_copy_bytes: every (destination, source) alignment pair, the sizes below two words, the word loop's
    second trip.  (tests/test_clips_capi.py checks that the table covers what it says.)"""
    rng = np.random.default_rng([47, COPY_SEED])
    nbytes = rng.choice(COPY_SIZES, 64)
    for f, v in COPY_BIG.items():
        nbytes[f] = v
    return _corpus(rng, nbytes, rng.integers(0, RAGGED_ISTRIDE, 64), COPY_STRIDE)


@functools.lru_cache(maxsize=None)
def corpus_many():
    """More files than k_corpus_copy's grid of 16384 workgroups."""
    rng = np.random.default_rng(53)
    F = 16384 + 3
    return _corpus(rng, rng.integers(0, 10, F), rng.integers(0, 3, F), 11)


def ragged_expected(c, pcap, icap):
    """-> (plan, payload bytes laid out, index entries laid out): the files' leading bytes and entries, in order."""
    plan = plan_of(c, pcap, icap)
    nb, ne = np.diff(plan[0]), np.diff(plan[1])
    pay = c.pay[np.arange(c.pay.shape[1])[None, :] < nb[:, None]]
    idx = c.index[np.arange(c.index.shape[1])[None, :] < ne[:, None]]
    return plan, pay, idx
