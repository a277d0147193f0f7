"""Inputs and the referee of the low-rate crop tests (tests/test_lowrate_capi.py, tests/test_gpu_lowrate.py): what
ulcx_decode_crops_lowrate_* (include/ulc_amd_lowrate.h) must give for a row.

The referee is the oracle's block loop (oracle/orc_decoder.c:156-201) restated around the oracle's own inverse transform
(lib.orc_imdct) at BlockSize BS' = BS >> lgD: for every sub-block of size S the transform buffer holds the leading S >> lgD of the S
coefficients the full decoder holds (File.coef, one oracle run), the window code is the block's own (File.wc), the overlap is
(S >> lgD) >> scale clipped to the previous sub-block's reduced size, the reversed-time FIFO centres decimated sub-blocks, and the
channel pairs are un-mixed after all channels.  At lgD 0 it is the oracle's decoder itself (File.pcm, bit for bit:
tests/test_lowrate_capi.py).  CPU only: numpy and the oracle; nothing here runs the library under test."""
import functools
import numpy as np
from ulc_testlib import oracle, ptr, f32p, to_pcm16
from corpus_testlib import Corpus, geom_files, oracle_file
from synth_spectra_testlib import code_stream, big_ref
import damage_testlib as D

POISON_F, POISON_I = 7.0, 7
DEAD_AT = 9                                                # the block the killed copy of a case's first file dies at

# The GPU cases: name -> (BlockSize, channels, lgD).  2048 x 2 down to 256 (k_dsyn, twiddles in LDS), 4096 x 2, 8192 x 2 (a walk of
# a non-fast geometry feeding the stereo kernel), mono, three and six channels (k_dgen), 32768 x 1 at 1/8, and the streams with
# every header code.
CASES = {
    "2048x2/2": (2048, 2, 1), "2048x2/4": (2048, 2, 2), "2048x2/8": (2048, 2, 3), "4096x2/2": (4096, 2, 1), "4096x2/4": (4096, 2, 2),
    "8192x2/2": (8192, 2, 1), "512x1/2": (512, 1, 1), "1024x1/4": (1024, 1, 2), "2048x3/2": (2048, 3, 1), "1024x6/4": (1024, 6, 2),
    "32768x1/8": (32768, 1, 3), "codes 2048x2/2": (2048, 2, 1), "codes 1024x1/4": (1024, 1, 2),
}


def blocks_of(bs, n_samples):
    """Blocks a sample crop of n_samples can touch (ulcx_crop_blocks)."""
    return 1 + (n_samples + bs - 2) // bs


@functools.lru_cache(maxsize=None)
def case_files(name):
    """The clean Files of a case, the first of them the one whose copy is killed at DEAD_AT.  Beside the shared streams of the
    geometry a case takes what its census (below) asks for: a high-quality stream for coded coefficients on both sides of the cut,
    a low-quality one for a noise tail that starts below it."""
    bs, ch, _ = CASES[name]
    if name.startswith("codes"):
        return (code_stream(bs, ch),) + tuple(geom_files((bs, ch))[:1])
    if (bs, ch) == (8192, 2):
        return (oracle_file(8192, 2, 40.0, 3, n_blocks=32), oracle_file(8192, 2, 95.0, 3, n_blocks=6))
    if (bs, ch) == (32768, 1):
        return (big_ref(), oracle_file(32768, 1, 95.0, 3, n_blocks=3), oracle_file(32768, 1, 4.0, 3, n_blocks=3))
    extra = {(1024, 1): ((1024, 1, 95.0, 11, 11, 12),), (4096, 2): ((4096, 2, 95.0, 3, 11, 8),), (1024, 6): ((1024, 6, 95.0, 3, 11, 8),)}.get((bs, ch), ())
    return tuple(geom_files((bs, ch))) + tuple(oracle_file(*e) for e in extra)


# ---------------------------------------------------------------------------------------------------------------------
# the referee
# ---------------------------------------------------------------------------------------------------------------------
def referee_blocks(coef, wc, bs, lgD):
    """coef [K][C][bs] under window codes wc [K] -> [K][bs >> lgD][C]: the oracle's decoder of BlockSize bs >> lgD from a fresh state,
    its transform buffer holding the low bins of every sub-block."""
    lib = oracle()
    K, C, _ = coef.shape
    bsr, H = bs >> lgD, (bs >> lgD) // 2
    out = np.zeros((K, bsr, C), np.float32)
    invlap = np.zeros((C, H), np.float32)
    tmp = np.zeros(4 * bsr, np.float32)
    last_sub = 0
    for k in range(K):
        w = int(wc[k])
        dst = np.zeros((C, bsr), np.float32)
        last = last_sub
        for ch in range(C):
            last = last_sub                                                     # :157
            lap = invlap[ch]
            pat = int(lib.orc_decimation_pattern(w))
            pos = dpos = 0
            while True:
                S = bs >> (pat & 7)
                Sr = S >> lgD
                tbuf = np.ascontiguousarray(coef[k, ch, pos:pos + Sr], np.float32)   # the leading S / D of the sub-block's S
                pos += S
                ov = Sr                                                         # :166-169
                if pat & 8:
                    ov >>= (w & 7)
                ov = min(ov, last)
                last = Sr
                if Sr == bsr:                                                   # :170
                    lib.orc_imdct(ptr(dst[ch], f32p), ptr(tbuf, f32p), ptr(lap, f32p), ptr(tmp, f32p), Sr, ov)
                    break
                dec = np.zeros(Sr, np.float32)
                lib.orc_imdct(ptr(dec, f32p), ptr(tbuf, f32p), ptr(lap, f32p), ptr(tmp, f32p), Sr, ov)
                avail = (bsr - Sr) // 2                                         # :173-185, the reversed-time FIFO: queue[q] = lap[H - 1 - q]
                queue = lap[::-1][:avail].copy()
                if Sr <= avail:
                    dst[ch, dpos:dpos + Sr] = queue[:Sr]
                    queue = np.concatenate([queue[Sr:], dec])
                else:
                    dst[ch, dpos:dpos + avail] = queue
                    dst[ch, dpos + avail:dpos + Sr] = dec[:Sr - avail]
                    queue = dec[Sr - avail:].copy()
                lap[H - avail:] = queue[::-1]
                dpos += Sr
                pat >>= 4
                if not pat:
                    break
        for ch in range(1, C, 2):                                               # :189-196, after all channels
            m, s = dst[ch - 1].copy(), dst[ch].copy()
            dst[ch - 1], dst[ch] = m + s, m - s
        out[k] = dst.T
        last_sub = last
    return out


_REF = {}


def referee(f, lgD):
    """A File's reduced stream [K][bs >> lgD][ch] (computed once per (file, ratio))."""
    key = (id(f), lgD)
    if key not in _REF:
        assert (f.obits > 0).all(), f.name
        _REF[key] = (f, referee_blocks(f.coef, f.wc, f.bs, lgD))
    return _REF[key][1]


# ---------------------------------------------------------------------------------------------------------------------
# corpora and rows
# ---------------------------------------------------------------------------------------------------------------------
class LowCase:
    """A case's corpus: its clean files and, last, a copy of file 0 with one dead block (DEAD_AT; damage_testlib's kill, under the clean
    index).  dead[f]: the block file f dies at, or None."""

    def __init__(self, name):
        self.name = name
        self.bs, self.ch, self.lgD = CASES[name]
        self.bsr = self.bs >> self.lgD
        files = list(case_files(name))
        st = D.Stream(files[0])
        self.dead_at = min(DEAD_AT, files[0].K - 2)
        killed, self.kill_seed = st.damage("kill", self.dead_at)
        self.cor = Corpus(files + [files[0]], payloads=[f.payload for f in files] + [killed])
        self.dead = [None] * len(files) + [self.dead_at]
        self.killed = killed

    def stream(self, f):
        """File f's reduced stream [ch][live blocks * bs'] and the sizes of its live blocks."""
        file = self.cor.files[f]
        live = file.K if self.dead[f] is None else self.dead[f]
        return referee(file, self.lgD)[:live].reshape(live * self.bsr, self.ch).T, file.obits[:live]

    def expected_row(self, f, start, n_samples, length=None, pcm16=False):
        """What row (f, start[, length]) must hold, as test_gpu_sample_crops.expected_row builds a sample-crop row: the file's reduced
        stream sliced at the sample, zeros behind the length, behind the file's end and from the dead block on; the sizes of the FULL
        blocks the row touches, 0 behind them.  A file number out of range, a negative start, a start more than a block past the
        indexed blocks, and a row whose block in front is the dead one give zeros."""
        bsr, ch, cor = self.bsr, self.ch, self.cor
        nB = blocks_of(bsr, n_samples)
        out, bits = np.zeros((ch, n_samples), np.float32), np.zeros(nB, np.int32)
        ln = n_samples if length is None else max(0, min(n_samples, int(length)))
        if 0 <= f < cor.F and start >= 0 and start // bsr <= cor.K[f] and ln > 0:
            stream, rb = self.stream(f)
            first = start // bsr
            if self.dead[f] is not None and first - 1 == self.dead[f]:
                return (to_pcm16(out) if pcm16 else out), bits               # the block in front is dead: the row never starts
            if self.dead[f] is not None and first > self.dead[f]:                # entered behind the dead block: the file is clean from there
                stream, rb = referee(cor.files[f], self.lgD).reshape(-1, ch).T, cor.files[f].obits
            end = min(start + ln, stream.shape[1])
            if end > start:
                out[:, :end - start] = stream[:, start:end]
            for b in range(first, (start + ln - 1) // bsr + 1):
                if b < len(rb):
                    bits[b - first] = rb[b]
        return (to_pcm16(out) if pcm16 else out), bits

    def switched(self, f):
        file = self.cor.files[f]
        return [k + 1 for k in range(file.K - 1) if int(file.wc[k]) != 0x10]

    def row_table(self, n_samples, total=24, seed=3):
        """(file, start, length) rows: starts at 0, at no multiple of anything, directly behind a switched block, inside the last
        block, at and beyond the file's end; lengths 0 and short; a bad file number; a negative start; rows over the dead block (ending
        at it, starting on it, starting behind it); then seeded starts up to `total`."""
        bsr, cor = self.bsr, self.cor
        K0, z, n = cor.K[0], cor.F - 1, n_samples
        sw = self.switched(0) or [1]
        d = self.dead_at
        t = [(0, 0, n), (0, bsr + bsr // 3 + 1, n), (0, sw[0] * bsr, n), (0, sw[-1] * bsr + 1, n), (0, (K0 - 1) * bsr + 5, n),
             (0, K0 * bsr, n), (0, (K0 + 1) * bsr + 3, n), (0, (K0 + 2) * bsr, n), (0, 2 * bsr + 7, 0), (0, 2 * bsr + 7, min(n, 3)),
             (0, bsr - 1, min(n, bsr + 2)), (cor.F, 0, n), (-1, 5, n), (0, -1, n), (0, -(1 << 40), n),
             (z, max(0, (d - 2) * bsr + 9), n), (z, (d - 1) * bsr + bsr - 1, n), (z, d * bsr + 1, n), (z, (d + 1) * bsr, n), (z, (d + 2) * bsr + 1, n)]
        rng = np.random.default_rng(seed)
        while len(t) < total:
            f = int(rng.integers(0, cor.F - 1))
            t.append((f, int(rng.integers(0, cor.K[f] * bsr)), n))
        return t[:max(total, 20)]


@functools.lru_cache(maxsize=None)
def low_case(name):
    return LowCase(name)


# ---------------------------------------------------------------------------------------------------------------------
# the census: what of the syntax the inputs of a case hold
# ---------------------------------------------------------------------------------------------------------------------
def unit_events(ny, pos, N):
    """The codes of one (channel, sub-block) unit of N coefficients from nybble `pos` of the block's nybbles `ny`, as the oracle's
    walk reads them (oracle/orc_decoder.c:57-125; the block is known to parse) -> ([(kind, first coefficient, count)], the position
    behind the unit): 'plain' - a run of coded coefficients no other code interrupts -, 'zero', 'noise' (8h), 'tail' (Fh,Fh), 'stop'."""
    ev, at = [], 0

    def quantizer():
        nonlocal pos
        q = int(ny[pos]); pos += 1
        if q == 0xF:
            return "tail"
        if q == 0xE:
            q += int(ny[pos]); pos += 1
        return "stop" if q == 0xE + 0xF else None

    esc = quantizer()
    esc = None if esc == "tail" else esc                    # (a unit that OPENS with Fh: a quantizer of 0.0, no tail - orc_decoder.c:48-54)
    plain = None                                            # the open run of coded coefficients
    while True:
        if esc is None:
            if at == N:
                break
            v = int(ny[pos]); pos += 1
            if v not in (0x0, 0x1, 0x8, 0xF):
                if plain is None:
                    plain = len(ev); ev.append(["plain", at, 0])
                ev[plain][2] += 1; at += 1
                continue
            plain = None
            if v == 0x0:
                n = int(ny[pos]) + 1; pos += 1
                ev.append(["zero", at, n]); at += n
            elif v == 0x1:
                n = ((int(ny[pos]) << 4) | int(ny[pos + 1])) + 33; pos += 2
                ev.append(["zero", at, n]); at += n
            elif v == 0x8:
                n = ((((int(ny[pos]) << 4) | int(ny[pos + 1])) << 1) | (int(ny[pos + 2]) & 1)) + 16; pos += 3
                ev.append(["noise", at, n]); at += n
            else:
                esc = quantizer()
            continue
        if esc == "tail":
            pos += 3
        ev.append([esc, at, N - at]); at = N
        break
    assert at == N
    return [tuple(e) for e in ev], pos


@functools.lru_cache(maxsize=None)
def census(name):
    """-> dict of counts over the case's clean files: codes (the header codes seen), plain_cross / run_cross / tail_cross (a run of
    plain coefficients, a noise run, a decaying-noise tail that starts below S >> lgD of its unit and ends at or above it),
    draws_max (the most noise draws of one unit)."""
    from spectra_testlib import subblocks_of
    bs, ch, lgD = CASES[name]
    out = dict(codes=set(), plain_cross=0, run_cross=0, tail_cross=0, draws_max=0)
    key = {"plain": "plain_cross", "noise": "run_cross", "tail": "tail_cross"}
    for f in case_files(name):
        for k in range(f.K):
            w = int(f.wc[k])
            out["codes"].add(w if w & 8 else w & 7)
            b = f.blocks[k, :f.nb[k] + 8]
            ny = np.empty(2 * b.size, np.uint8)
            ny[0::2], ny[1::2] = b & 15, b >> 4             # low nybble first
            pos = 2 if w & 8 else 1
            for c in range(ch):
                for S in subblocks_of(bs, w):
                    ev, pos = unit_events(ny, pos, S)
                    cut = S >> lgD
                    out["draws_max"] = max(out["draws_max"], sum(n for kind, _, n in ev if kind in ("noise", "tail")))
                    for kind, a, n in ev:
                        if kind in key and a < cut <= a + n - 1:
                            out[key[kind]] += 1
            assert (pos + 1) // 2 == f.nb[k], (f.name, k, pos, f.nb[k])     # the walk ends where the oracle's size says
    return out
