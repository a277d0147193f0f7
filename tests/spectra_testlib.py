"""Inputs and oracle references of the spectra tests (tests/test_spectra_capi.py, tests/test_gpu_spectra.py): what
ulcx_decode_crops_spectra_* must give for a row - the dequantised coefficients the oracle's decoder holds for every block
(orc_decode_stream_coefs / CoefDbg), channels-first; the window codes from each block's first byte; the oracle's sizes - and
the properties of the test streams the GPU tests rely on, counted with the decoder written from FormatSpecs.md alone
(tests/spec_decoder.py).  CPU only; nothing here runs the library under test."""
import ctypes as C
import functools
import numpy as np
from ulc_testlib import oracle, synth_pcm, oracle_encode_debug, same_bits, wc_of
from seek_testlib import RATE, oracle_stream
from corpus_testlib import File, Corpus, geom_files, to_lr
from spec_decoder import _WINDOWS, decode_block_coefficients

SPECTRA_LR = 1
N_BLOCKS = 5                                               # blocks per row of the row tests
DECIMATED = {(8, 8, 4, 2), (4, 8, 8, 2), (2, 8, 8, 4), (2, 4, 8, 8)}


def subblocks_of(bs, wc):
    """Sub-block sizes, in coded order, of a block with window code wc, from the oracle's pattern table (ulcDecoder.c:219-245)."""
    pat = int(oracle().orc_decimation_pattern(int(wc)))
    out = []
    while True:
        out.append(bs >> (pat & 7))
        if out[-1] == bs:
            return (bs,)
        pat >>= 4
        if not pat:
            return tuple(out)


@functools.lru_cache(maxsize=None)
def geom_corpus(geom):
    """The oracle-encoded and hand-assembled streams of a geometry of seek_testlib.geometries(), together in one corpus."""
    return Corpus(geom_files(geom))


def row_table(cor, n_blocks=N_BLOCKS):
    """(file, first) rows over a corpus: first 0, first 1, starts directly behind window-switched blocks, a start two blocks before
    the file's end, first = the block count, several rows naming one file - every file of the corpus takes each."""
    rows = []
    for f, fs in enumerate(cor.files):
        sw = [k + 1 for k in range(fs.K - 1) if int(fs.wc[k]) != 0x10]
        assert len(sw) >= 2, fs.name
        rows += [(f, 0), (f, 1), (f, sw[0]), (f, sw[len(sw) // 2]), (f, sw[-1]), (f, fs.K - 2), (f, fs.K)]
    return rows


def seventy_rows(cor, n_blocks=N_BLOCKS, seed=5):
    """70 rows (more than a wave of the walk has lanes): row_table(), then seeded (file, first) pairs."""
    rows = row_table(cor, n_blocks)
    rng = np.random.default_rng(seed)
    while len(rows) < 70:
        f = int(rng.integers(0, cor.F))
        rows.append((f, int(rng.integers(0, cor.K[f] + 1))))
    return rows[:70]


def noise_pass_rows():
    """Rows of N_BLOCKS blocks of the oracle-encoded 4096 x 2 file (file 0 of its corpus) that between them hold every block with a
    unit of more than 2048 noise coefficients (tests/test_spectra_capi.py asserts that they do)."""
    return [(0, first) for first in (2, 6, 12, 17, 22, 32, 35)]


# ---------------------------------------------------------------------------------------------------------------------
# what the streams hold, by the decoder written from the format's text
# ---------------------------------------------------------------------------------------------------------------------
def _spec_sizes(bs, wc):
    wc = int(wc)
    return [bs // d for d in _WINDOWS[wc >> 4]] if wc & 8 else [bs]


@functools.lru_cache(maxsize=None)
def _census(key):
    blocks, bits, ch, bs = _CENSUS_INPUT[key]
    out = []
    for k in range(blocks.shape[0]):
        wc = int(wc_of(blocks[k:k + 1])[0])
        sizes = _spec_sizes(bs, wc)
        coef, noise, _ = decode_block_coefficients(blocks[k, :(int(bits[k]) + 7) // 8], ch, bs)
        units, off = [], 0
        for c in range(ch):
            off = 0
            for S in sizes:
                nz = noise[c, off:off + S] > 0
                coded = (coef[c, off:off + S] != 0) & ~nz
                edges = np.flatnonzero(np.diff(np.concatenate([[0], coded.astype(np.int8), [0]])))
                runs = edges[1::2] - edges[0::2]
                units.append(dict(ch=c, S=S, noise=int(nz.sum()), coded=int(coded.sum()), records=int(((runs + 6) // 7).sum())))
                off += S
        out.append(dict(wc=wc, shape=tuple(bs // S for S in sizes), units=units))
    return out


_CENSUS_INPUT = {}


def census(name, blocks, bits, ch, bs):
    """Per block of an oracle-encoded stream: its window code, its shape (the divisors of its sub-blocks, (1,) for a full block) and
    per (channel, sub-block) unit the noise coefficients, the coded coefficients and a LOWER bound of the walk's plain-run records
    (maximal runs of consecutive coded coefficients, cut every 7: a quantizer change inside a run only adds records)."""
    _CENSUS_INPUT[name] = (blocks, np.asarray(bits), ch, bs)
    return _census(name)


@functools.lru_cache(maxsize=None)
def big_stream(ch, transient, n_blocks=3, q=30.0, sid=3):
    """A BlockSize 32768 file of n_blocks blocks -> File.  transient=False: tones and noise only - its blocks stay un-decimated."""
    bs = 32768
    if transient:
        blocks, bits, _ = oracle_stream(bs, ch, q, sid, n_blocks=n_blocks)
    else:
        pcm = synth_pcm(sid, n_blocks * bs, ch, RATE, transient=False, seed=11)
        r = oracle_encode_debug(pcm, bs, RATE, 0, q, slot=2 * ch * bs + 16)
        blocks, bits = r["out"], r["bits"]
    return File(f"oracle 32768x{ch} q{q:g} {'transient' if transient else 'steady'}", bs, ch, blocks, bits)


# ---------------------------------------------------------------------------------------------------------------------
# damaged payloads: the oracle block by block, as tests/damage_testlib.py's model runs it, handing back coefficients
# ---------------------------------------------------------------------------------------------------------------------
class _OrcDecoder(C.Structure):
    """orc_decoder (oracle/ulc_oracle.h)."""
    _fields_ = [("nChan", C.c_int), ("BlockSize", C.c_int), ("LastSubBlockSize", C.c_int), ("Seed", C.c_uint32),
                ("TransformBuffer", C.c_void_p), ("TransformTemp", C.c_void_p), ("TransformInvLap", C.c_void_p), ("CoefDbg", C.c_void_p)]


def oracle_coefs_seeded(rows, ch, bs, seed):
    """The oracle's decoder over slot-form rows [m][slot] from generator state `seed`, block by block, until a block gives 0 bits
    -> (coef [m][ch][bs], bits [m]); blocks from the failing one on are zeros."""
    lib = oracle()
    lib.orc_decoder_init.argtypes = [C.POINTER(_OrcDecoder)]
    lib.orc_decoder_destroy.argtypes = [C.POINTER(_OrcDecoder)]
    lib.orc_decoder_destroy.restype = None
    lib.orc_decode_block.argtypes = [C.POINTER(_OrcDecoder), C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, np.uint8)
    m = rows.shape[0]
    coef, bits = np.zeros((m, ch, bs), np.float32), np.zeros(m, np.int32)
    st = _OrcDecoder()
    st.nChan, st.BlockSize = ch, bs
    assert lib.orc_decoder_init(C.byref(st)) >= 0
    st.Seed = int(seed)
    pcm = np.zeros(ch * bs, np.float32)
    try:
        for k in range(m):
            b = lib.orc_decode_block(C.byref(st), pcm.ctypes.data, rows[k].ctypes.data)
            if b <= 0:
                break
            bits[k] = b
            coef[k] = np.ctypeslib.as_array(C.cast(st.CoefDbg, C.POINTER(C.c_float)), (ch, bs))
    finally:
        lib.orc_decoder_destroy(C.byref(st))
    return coef, bits


def damaged_row(payload, offs, rng_states, ch, bs, first, n):
    """What a spectra row of n blocks from `first` must give for a file whose bytes changed behind its index (damage_testlib's
    model, with coefficients for samples): blocks first - 1 .. first + n - 1 each read at their index offset and cut to their index
    extent, decoded from the stored generator state of the first of them; a block of 0 bits, or of more bits than its extent, ends
    the row - the block in front included.  -> (coef [ch][n][bs], wc [n], bits [n], live)."""
    K = len(offs) - 1
    coef, wc, bits = np.zeros((ch, n, bs), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    if first < 0 or first > K:
        return coef, wc, bits, 0
    k0, k1 = max(first - 1, 0), min(first + n, K)
    m = k1 - k0
    if m <= 0 or k1 <= first:
        return coef, wc, bits, 0
    slot = 2 * ch * bs + 16
    rows = np.zeros((m, slot), np.uint8)
    ext = np.zeros(m, np.int64)
    for i in range(m):
        a, b = int(offs[k0 + i]), int(offs[k0 + i + 1])
        rows[i, :b - a] = payload[a:b]
        ext[i] = b - a
    oc, ob = oracle_coefs_seeded(rows, ch, bs, int(rng_states[k0]))
    alive = 0
    while alive < m and 0 < ob[alive] <= 8 * ext[alive]:
        alive += 1
    warm = first - k0
    live = max(0, alive - warm)
    coef[:, :live] = oc[warm:warm + live].transpose(1, 0, 2)
    wc[:live] = wc_of(rows[warm:warm + live])
    bits[:live] = ob[warm:warm + live]
    return coef, wc, bits, live
