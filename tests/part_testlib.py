"""Inputs and expected rows of the mid / side crop tests (tests/test_part_capi.py, tests/test_gpu_part.py): what
ulcx_decode_crops_part_* (include/ulc_amd_part.h) must give for a row.

Output plane j of a row is coded channel 2 j + part as the reference decoder holds it in DstData in front of its un-mix loop
(ulcDecoder.c:279-289).  The referee is lowrate_testlib.referee_blocks - the oracle's block loop around the oracle's inverse
transform at BlockSize BS >> lgD - called with ONE channel, coef[:, ch:ch + 1, :]: a one-channel reference decoder that holds that
channel's planes and un-mixes nothing.  It is called per channel, never with two picked channels at once (it un-mixes pairs).
The rows are built as lowrate_testlib.LowCase.expected_row builds them: the same files (lowrate_testlib.case_files, code_stream)
and beside them one stream with a silent stretch and a click, the same killed copy, a row table like LowCase.row_table's.
CPU only: numpy and the oracle; nothing here runs the library under test."""
import functools
import numpy as np
from ulc_testlib import oracle_encode_debug, oracle_decode_stream, synth_pcm, to_pcm16
from corpus_testlib import Corpus, File, oracle_file
from spectra_testlib import subblocks_of
import damage_testlib as D
import lowrate_testlib as LT
from lowrate_testlib import POISON_F, POISON_I, DEAD_AT, blocks_of, referee_blocks, unit_events   # noqa: F401 (the tests' names)

MID, SIDE = 0, 1
RATE = 44100

# The cases: name -> (BlockSize, channels, lgD, codes).  Each is the smallest that reaches a pick of the synthesis:
#   256x2/0, 1024x2/1            stereo below 2048 (where a stereo kernel keeps its twiddles in LDS)
#   2048x2/0, /1, /3             the constant-BlockSize geometry and reduced ones
#   4096x2/0, /1                 stereo without twiddles in LDS
#   8192x2/1                     a walk of a non-stereo-kernel geometry feeding a reduced geometry that has one
#   8192x2/0, 512x1/0, 2048x3/1, 1024x6/2   the general kernel's own geometries: the mono identity, the unpaired last channel
#   codes 2048x2/1, codes 1024x1/0          every header code
CASES = {
    "256x2/0": (256, 2, 0, False), "1024x2/1": (1024, 2, 1, False),
    "2048x2/0": (2048, 2, 0, False), "2048x2/1": (2048, 2, 1, False), "2048x2/3": (2048, 2, 3, False),
    "4096x2/0": (4096, 2, 0, False), "4096x2/1": (4096, 2, 1, False),
    "8192x2/1": (8192, 2, 1, False), "8192x2/0": (8192, 2, 0, False),
    "512x1/0": (512, 1, 0, False), "2048x3/1": (2048, 3, 1, False), "1024x6/2": (1024, 6, 2, False),
    "codes 2048x2/1": (2048, 2, 1, True), "codes 1024x1/0": (1024, 1, 0, True),
}


def part_channels(ch, part):
    """ulcx_part_channels, restated."""
    return (ch + 1 - part) // 2 if part in (MID, SIDE) and 1 <= ch <= 255 else 0


def parts_of(ch):
    return [p for p in (MID, SIDE) if part_channels(ch, p)]


@functools.lru_cache(maxsize=None)
def gap_file(bs, ch):
    """An oracle-encoded stream of 16 blocks with what the shared streams need not have: a click inside block 3 (decimated blocks
    around it, whatever the BlockSize) and silence over blocks 8 .. 10 (at least one block without a coefficient, and an onset
    behind it).  Quality 30: noise fill in every channel of the loud blocks."""
    n = 16 * bs
    pcm = synth_pcm(5, n, ch, RATE, transient=False, seed=21).copy()
    rng = np.random.default_rng(77)
    ln = min(3000, 2 * bs)
    at = 3 * bs + bs // 3
    burst = (rng.normal(0, 0.4, ln) * np.exp(-np.arange(ln) / (ln / 10.0))).astype(np.float32)
    for c in range(ch):
        pcm[at:at + ln, c] += (0.8 ** c) * burst
    pcm[8 * bs:11 * bs] = 0.0
    pcm = np.clip(pcm, -1.0, 32767.0 / 32768.0).astype(np.float32)
    r = oracle_encode_debug(pcm, bs, RATE, 0, 30.0, slot=2 * ch * bs + 16)
    rc, _, bits = oracle_decode_stream(r["out"], ch, bs)
    assert rc == 0
    return File(f"gap {bs}x{ch}", bs, ch, r["out"], bits)


@functools.lru_cache(maxsize=None)
def case_files(name):
    """The clean Files of a case, the first of them the one whose copy is killed: the low-rate family's files of the geometry where
    it has a case of it (lowrate_testlib.case_files), else two oracle streams of 32 and 8 blocks; then the geometry's gap_file."""
    bs, ch, _, codes = CASES[name]
    twin = next((n for n, (b, c, _) in LT.CASES.items() if (b, c) == (bs, ch) and n.startswith("codes") == codes), None)
    files = LT.case_files(twin) if twin else (oracle_file(bs, ch, 50.0, 3, n_blocks=32), oracle_file(bs, ch, 95.0, 3, 11, 8))
    return tuple(files) + (gap_file(bs, ch),)


# ---------------------------------------------------------------------------------------------------------------------
# the referee, per coded channel
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def channel_plane(f, lgD, ch):
    """Coded channel ch of File f as a one-channel reference decoder of BlockSize bs >> lgD holds it: [K][bs >> lgD]."""
    key = (id(f), lgD, ch)
    if key not in _REF:
        assert (f.obits > 0).all(), f.name
        _REF[key] = (f, referee_blocks(np.ascontiguousarray(f.coef[:, ch:ch + 1, :]), f.wc, f.bs, lgD)[:, :, 0])
    return _REF[key][1]


def decimated(f, k):
    return len(subblocks_of(f.bs, int(f.wc[k]))) > 1


class PartCase:
    """A case's corpus: its clean files and, last, a copy of file 0 with one dead block (DEAD_AT; damage_testlib's kill, under the
    clean index), as lowrate_testlib.LowCase.  dead[f]: the block file f dies at, or None."""

    def __init__(self, name):
        self.name = name
        self.bs, self.ch, self.lgD, _ = CASES[name]
        self.bsr = self.bs >> self.lgD
        files = list(case_files(name))
        st = D.Stream(files[0])
        self.dead_at = min(DEAD_AT, files[0].K - 2)
        killed, self.kill_seed = st.damage("kill", self.dead_at)
        self.cor = Corpus(files + [files[0]], payloads=[f.payload for f in files] + [killed])
        self.dead = [None] * len(files) + [self.dead_at]
        self.gap = len(files) - 1                              # the gap file's number

    def planes(self, f, part, live=None):
        """File f's reduced planes of `part`, [nOut][live blocks * bs'] (live: all blocks)."""
        file = self.cor.files[f]
        live = file.K if live is None else live
        return np.stack([channel_plane(file, self.lgD, c)[:live].reshape(-1) for c in range(part, self.ch, 2)])

    def expected_row(self, f, start, n_samples, length, part, pcm16=False):
        """What row (f, start[, length]) of a call with `part` must hold (LowCase.expected_row over the part's planes): the planes
        sliced at the sample, zeros behind the length, behind the file's end and from the dead block on; the sizes of the FULL blocks
        the row touches, 0 behind them.  A file number out of range, a negative start, a start more than a block past the indexed
        blocks, and a row whose block in front is the dead one give zeros."""
        bsr, cor = self.bsr, self.cor
        nB = blocks_of(bsr, n_samples)
        out, bits = np.zeros((part_channels(self.ch, part), n_samples), np.float32), np.zeros(nB, np.int32)
        ln = n_samples if length is None else max(0, min(n_samples, int(length)))
        if 0 <= f < cor.F and start >= 0 and start // bsr <= cor.K[f] and ln > 0:
            first = start // bsr
            dead = self.dead[f]
            if dead is not None and first - 1 == dead:
                return (to_pcm16(out) if pcm16 else out), bits               # the block in front is dead: the row never starts
            live = dead if dead is not None and first <= dead else cor.K[f]  # (entered behind the dead block: the file is clean from there)
            stream, rb = self.planes(f, part, live), cor.files[f].obits[:live]
            end = min(start + ln, stream.shape[1])
            if end > start:
                out[:, :end - start] = stream[:, start:end]
            for b in range(first, (start + ln - 1) // bsr + 1):
                if b < len(rb):
                    bits[b - first] = rb[b]
        return (to_pcm16(out) if pcm16 else out), bits

    def behind_decimated(self):
        """(file, block) pairs whose block in front is decimated, clean files only."""
        return [(f, k + 1) for f in range(self.cor.F - 1) for k in range(self.cor.K[f] - 1) if decimated(self.cor.files[f], k)]

    def row_table(self, n_samples, total=24, seed=3):
        """(file, start, length) rows, as LowCase.row_table: starts at a block edge, one sample past it, in the last sample of a block,
        directly behind a decimated block, inside the last block, at and beyond the file's end; lengths 0 and short; a file named
        twice (file 0, many times); bad file numbers; negative starts; rows over the dead block (ending at it, starting on it, one
        whose block in front is the dead one, one entering behind it); the silent stretch; then seeded starts up to `total`."""
        bsr, cor = self.bsr, self.cor
        K0, z, g, n = cor.K[0], cor.F - 1, self.gap, n_samples
        bf, bk = self.behind_decimated()[0]
        d = self.dead_at
        t = [(0, 0, n), (0, 2 * bsr, n), (0, 2 * bsr + 1, n), (0, 3 * bsr - 1, n), (bf, bk * bsr, n), (bf, bk * bsr + 1, n), (0, (K0 - 1) * bsr + 5, n),
             (0, K0 * bsr, n), (0, (K0 + 1) * bsr + 3, n), (0, 2 * bsr + 7, 0), (0, 2 * bsr + 7, min(n, 3)), (0, bsr - 1, min(n, bsr + 2)),
             (cor.F, 0, n), (-1, 5, n), (0, -1, n), (0, -(1 << 40), n),
             (z, max(0, (d - 2) * bsr + 9), n), (z, d * bsr + 1, n), (z, (d + 1) * bsr, n), (z, (d + 2) * bsr + 1, n),
             (g, 7 * bsr + 3, n), (g, 9 * bsr, n)]
        rng = np.random.default_rng(seed)
        while len(t) < total:
            f = int(rng.integers(0, cor.F - 1))
            t.append((f, int(rng.integers(0, cor.K[f] * bsr)), n))
        return t


@functools.lru_cache(maxsize=None)
def part_case(name):
    return PartCase(name)


# ---------------------------------------------------------------------------------------------------------------------
# the census: what the inputs of a case hold
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census(name):
    """-> dict of counts over the case's clean files: whole / decimated (blocks of one / several sub-blocks), side_after_mid (blocks in
    which a channel 2 j + 1 draws noise and the channel 2 j in front of it drew noise too: a side state taken from the block's start
    gives other signs), silent (blocks without one coefficient or draw), behind_decimated (blocks a row can start in whose block in
    front is decimated)."""
    bs, ch, _, _ = CASES[name]
    out = dict(whole=0, decimated=0, side_after_mid=0, silent=0, behind_decimated=0)
    for f in case_files(name):
        for k in range(f.K):
            w = int(f.wc[k])
            subs = subblocks_of(bs, w)
            out["decimated" if len(subs) > 1 else "whole"] += 1
            out["behind_decimated"] += 1 if k + 1 < f.K and len(subs) > 1 else 0
            b = f.blocks[k, :f.nb[k] + 8]
            ny = np.empty(2 * b.size, np.uint8)
            ny[0::2], ny[1::2] = b & 15, b >> 4             # low nybble first
            pos = 2 if w & 8 else 1
            draws, coded = [], 0
            for c in range(ch):
                dr = 0
                for S in subs:
                    ev, pos = unit_events(ny, pos, S)
                    dr += sum(n for kind, _, n in ev if kind in ("noise", "tail"))
                    coded += sum(n for kind, _, n in ev if kind == "plain")
                draws.append(dr)
            assert (pos + 1) // 2 == f.nb[k], (f.name, k, pos, f.nb[k])     # the walk ends where the oracle's size says
            out["side_after_mid"] += 1 if any(draws[c] > 0 and draws[c - 1] > 0 for c in range(1, ch, 2)) else 0
            out["silent"] += 1 if coded == 0 and sum(draws) == 0 else 0
    return out
