"""Inputs and oracle references of the clip tests (tests/test_clips_capi.py, tests/test_gpu_clips.py): channels-first clips of
different length, what the oracle's encoder writes for each clip alone (oracle_encode_debug of the interleaved clip zero-padded to
the tool's block count), the index of that payload from the oracle's decoder (seek_testlib.oracle_walk), and the numpy
restatement of ulcx_corpus_ragged_dev's offsets and capacity rule.  CPU only."""
import functools
import numpy as np
from ulc_testlib import synth_pcm, oracle_encode_debug, oracle_decode_stream
from seek_testlib import oracle_walk, SEED0
from rates_testlib import mode_of

RATE = 44100
GEOMS = [(256, 2), (512, 1), (256, 3)]                      # the stereo vector path, mono, the generic channel loop
INDEX_DTYPE = np.dtype([("ByteOffs", np.int32), ("RngState", np.uint32)])
SCALAR = (-50.0, 0.0)                                       # VBR 50 in the tool's convention
TABLE = [(-50.0, 0.0), (64.0, 0.0), (96.0, 1.5), (-30.0, 0.0), (48.0, 0.0), (80.0, 2.0), (-70.0, 0.0)]     # VBR, CBR and ABR rows mixed


def clip_blocks(bs, n):
    """The tool's block count for a file of n samples (tools/ulcEncodeTool.c:93-98); 0 for an empty clip."""
    return (n + bs - 1) // bs + 2 if n >= 1 else 0


def n_samples(bs):
    return 5 * bs + 3                                       # odd: the planes of rows and channels start at every alignment


def lengths(bs):
    return [0, 1, bs - 1, bs, bs + 1, 3 * bs + 7, n_samples(bs)]


@functools.lru_cache(maxsize=None)
def wave(bs, ch):
    """[7][ch][nSamples] float32 on the PCM16 grid: synth_pcm per row, transposed.  Samples behind a row's length are NOT zero:
    the call must not read them into the clip."""
    T = n_samples(bs)
    return np.stack([np.ascontiguousarray(synth_pcm(20 + i, T, ch, RATE, transient=True, seed=17).T) for i in range(7)])


class ClipRef:
    """One clip under one setting, from the oracle alone: blocks, sizes, payload, index row."""

    def __init__(self, bs, ch, clip, setting):
        L = clip.shape[1]
        self.bs, self.ch, self.L, self.nb = bs, ch, L, clip_blocks(bs, L)
        self.slot = 2 * ch * bs + 16
        if self.nb == 0:
            self.blocks, self.bits = np.zeros((0, self.slot), np.uint8), np.zeros(0, np.int32)
        else:
            pcm = np.zeros((self.nb * bs, ch), np.float32)
            pcm[:L] = clip.T
            mode, p0, p1 = mode_of(setting)
            r = oracle_encode_debug(pcm, bs, RATE, mode, p0, p1, slot=self.slot)
            self.blocks, self.bits = r["out"], r["bits"]
            assert (self.bits > 0).all() and (self.bits % 8 == 0).all()
        self.sizes = self.bits.astype(np.int64) // 8
        self.payload = (np.concatenate([self.blocks[k, :self.sizes[k]] for k in range(self.nb)]) if self.nb else np.zeros(0, np.uint8)).astype(np.uint8)

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
        nbytes = int(self.sizes[:m].sum())
        row = np.zeros(index_stride, INDEX_DTYPE)
        row["ByteOffs"] = -1
        row["ByteOffs"][0], row["RngState"][0] = 0, SEED0
        if m:
            wbits, offs, seeds, inside = oracle_walk(self.payload, nbytes, self.ch, self.bs, index_stride - 1)
            assert inside and len(wbits) == m and np.array_equal((wbits + 7) // 8, self.sizes[:m])      # the oracle's decoder reads back the oracle's encoder
            row["ByteOffs"][:m + 1], row["RngState"][:m + 1] = offs, seeds
        return row

    def decoded(self):
        """[nb * bs][ch]: the oracle's sequential decode of the blocks."""
        rc, pcm, _ = oracle_decode_stream(self.blocks, self.ch, self.bs)
        assert rc == 0
        return pcm


@functools.lru_cache(maxsize=None)
def refs(bs, ch, table=False, pcm16=False):
    """The seven rows' references under the scalar setting or the mixed table."""
    w, L = wave(bs, ch), lengths(bs)
    return [ClipRef(bs, ch, w[i][:, :L[i]], TABLE[i] if table else SCALAR) for i in range(7)]


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
