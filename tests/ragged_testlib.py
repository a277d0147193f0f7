"""Inputs and oracle references of the ragged-corpus tests (tests/test_gpu_crops_ragged*.py): files of very different length
per geometry, what the oracle says of each (tests/seek_testlib.py), and the two layouts of a corpus built from them - the
ragged one (payloads and index rows back to back behind int64 offset tables) and its strided copy.  CPU only."""
import functools
import numpy as np
from seek_testlib import oracle_stream, oracle_seeds, oracle_pcm, expected_range

FILE_BLOCKS = (1, 2, 7, 12, 40)
# geometry -> (VBR quality, synth_pcm stream id of the 40-block file: the stream of seek_testlib.ORACLE_CASES; the shorter files
# take the ids behind it).  Stereo 2048 runs the specialised synthesis, the other two the general one.
GEOMS = {(2048, 2): (50.0, 3), (1024, 1): (20.0, 11), (2048, 3): (60.0, 3)}
PAD = 64                                                   # bytes behind the last payload (corpus.PAYLOAD_PAD)
INDEX_DTYPE = np.dtype([("ByteOffs", np.int32), ("RngState", np.uint32)])


class FileRef:
    """One file: its packed payload and, from the oracle alone, its index (offsets, generator states) and its decode."""

    def __init__(self, bs, ch, blocks, bits):
        self.bs, self.ch, self.K = bs, ch, len(bits)
        nb = (bits.astype(np.int64) + 7) // 8
        self.payload = np.concatenate([blocks[k, :nb[k]] for k in range(self.K)]).astype(np.uint8)
        self.offs = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        self.seeds = oracle_seeds(blocks, ch, bs)
        self.pcm, self.bits = oracle_pcm(blocks, ch, bs)

    def row(self, cap=None, blocks=None):
        """The file's index row of `cap` entries (default: blocks + 1) as the index calls fill one: the first `blocks` blocks,
        {-1, 0} behind the closing entry."""
        n = self.K if blocks is None else blocks
        cap = n + 1 if cap is None else cap
        r = np.zeros(cap, INDEX_DTYPE)
        r["ByteOffs"] = -1
        r["ByteOffs"][:n + 1] = self.offs[:n + 1]
        r["RngState"][:n + 1] = self.seeds[:n + 1]
        return r

    def expected(self, first, N, count=None):
        want, wb = expected_range(self.pcm, self.bits, int(first), N)
        if count is not None:
            m = max(0, min(N, int(count)))
            want[m:] = 0; wb[m:] = 0
        return want, wb


@functools.lru_cache(maxsize=None)
def file_refs(geom):
    bs, ch = geom
    q, sid = GEOMS[geom]
    out = []
    for i, K in enumerate(FILE_BLOCKS):
        blocks, bits, _ = oracle_stream(bs, ch, q, sid) if K == 40 else oracle_stream(bs, ch, q, sid + 1 + i, 11, K)
        assert (bits > 0).all()
        out.append(FileRef(bs, ch, blocks, bits))
    return out


class Ragged:
    """files: FileRefs, or None for a file nobody crops (no payload bytes, a row of one entry).  -> payload uint8 [total + PAD],
    payload_offs / index_offs int64 [F + 1], index [entries] (row f: blocks_f + 1), index_blocks int32 [F]."""

    def __init__(self, files):
        self.files, self.F = list(files), len(files)
        sizes = [0 if f is None else f.payload.size for f in files]
        caps = [1 if f is None else f.K + 1 for f in files]
        self.poffs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.ioffs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        self.payload = np.zeros(int(self.poffs[-1]) + PAD, np.uint8)
        self.index = np.zeros(int(self.ioffs[-1]), INDEX_DTYPE)
        self.blocks = np.array([0 if f is None else f.K for f in files], np.int32)
        for i, f in enumerate(files):
            if f is None:
                self.index[self.ioffs[i]] = (0, 1234567)
            else:
                self.payload[self.poffs[i]:self.poffs[i + 1]] = f.payload
                self.index[self.ioffs[i]:self.ioffs[i + 1]] = f.row()

    def strided(self):
        """The same corpus in the strided layout -> (payload [F][stride], payload_bytes, index [F][index_stride], index_blocks)."""
        sizes = np.diff(self.poffs)
        stride = (int(sizes.max()) + PAD + 15) & ~15
        istride = int(np.diff(self.ioffs).max())
        host = np.zeros((self.F, stride), np.uint8)
        index = np.zeros((self.F, istride), INDEX_DTYPE)
        index["ByteOffs"] = -1
        for i in range(self.F):
            host[i, :sizes[i]] = self.payload[self.poffs[i]:self.poffs[i + 1]]
            index[i, :self.ioffs[i + 1] - self.ioffs[i]] = self.index[self.ioffs[i]:self.ioffs[i + 1]]
        return host, sizes.astype(np.int32), index, self.blocks.copy()

    def expected(self, files, first, N, count=None):
        """-> (pcm [n][N][bs][ch], bits [n][N]) of the rows; a file number outside the corpus, or a None file, gives zeros."""
        ref = next(f for f in self.files if f is not None)
        pcm = np.zeros((len(files), N, ref.bs, ref.ch), np.float32)
        bits = np.zeros((len(files), N), np.int32)
        for i, f in enumerate(files):
            if 0 <= f < self.F and self.files[f] is not None and 0 <= first[i] <= self.files[f].K:
                pcm[i], bits[i] = self.files[f].expected(first[i], N, None if count is None else count[i])
        return pcm, bits


def to_pcm16(x):
    return np.clip(np.rint(x.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)       # WavIO_Helper.c:56-63


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()
