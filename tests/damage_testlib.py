"""Inputs and oracle references of the damaged-payload tests (tests/test_damage_model.py, tests/test_gpu_damaged_crops.py): a
payload whose bytes changed after its block index was written, and what a range, crop or sample-crop call must give for it.

The model (local_model) is what include/ulc_amd.h promises of such a call, carried out with the oracle's decoder alone: the
blocks first-1 .. first+n-1 are each read at their index offset and cut to their index extent (zeros behind it), decoded from a
fresh decoder whose generator word is the stored RngState of the first of them; the block in front of the range gives the
lapping state and no output; a block for which the oracle reports 0 bits, or more bits than its extent holds, ends the row -
zero samples and 0 bits from it on.  The damages are single nybbles of one block, sorted by what the model says of them: a kill
ends the row, a value damage changes samples and no size ('draws': it also changes the block's number of noise draws, so the
generator is displaced behind it), a resize changes the block's size and leaves the row alive.
CPU only; nothing here runs the library under test."""
import ctypes as C
import functools
import numpy as np
from ulc_testlib import oracle, ptr, f32p, i32p, u8p, to_pcm16, same_bytes
from seek_testlib import geometries
from corpus_testlib import File, Corpus, geom_files, oracle_file

MAX_SEED = 400
EXTRA = {(1024, 2): (50.0, 3)}                             # stereo below BlockSize 2048: no geometry of seek_testlib's has it
GEOMS = sorted(set(geometries().keys()) | set(EXTRA))      # the six of seek_testlib and 1024 x 2
KINDS = ("kill", "value", "draws", "resize")                # a geometry's damaged copies per position; 'draws' and 'resize' where a seed gives one
POSITIONS = (6, 7)                                         # damaged blocks of every geometry; switched_position() adds one


def _lib():
    lib = oracle()
    lib.orc_decode_stream_seeded.argtypes = [C.c_int, C.c_int, u8p, C.c_int, C.c_int, f32p, i32p, C.POINTER(C.c_uint32)]
    return lib


def blocks_of(bs, n_samples):
    """Blocks a sample crop of n_samples can touch (ulcx_crop_blocks)."""
    return 1 + (n_samples + bs - 2) // bs


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def local_model(payload, offs, rng_states, ch, bs, first, n):
    """-> (pcm float32 [n][bs][ch], bits int32 [n], live): blocks first .. first+n-1 of the file `payload` (uint8, 1-D) under
    the index (offs [K+1], rng_states [K+1]).  live: the row's leading blocks that are decoded - the row ends in front of block
    first + live (at a dead block, at the file's end, or with live == n); 0 where the block in front of the range is dead or
    `first` lies outside [0, K]."""
    K = len(offs) - 1
    pcm, bits = np.zeros((n, bs, ch), np.float32), np.zeros(n, np.int32)
    if first < 0 or first > K or n <= 0:
        return pcm, bits, 0
    k0, k1 = max(first - 1, 0), min(first + n, K)
    m = k1 - k0
    if m <= 0 or k1 <= first:
        return pcm, bits, 0
    slot = 2 * ch * bs + 16
    rows = np.zeros((m, slot), np.uint8)
    ext = np.zeros(m, np.int64)
    for i in range(m):
        a, b = int(offs[k0 + i]), int(offs[k0 + i + 1])
        assert 0 <= a < b <= len(payload) and b - a <= slot - 16, (a, b)
        rows[i, :b - a] = payload[a:b]
        ext[i] = b - a
    op, ob = np.zeros((m * bs, ch), np.float32), np.zeros(m, np.int32)
    sd = C.c_uint32(int(rng_states[k0]))
    _lib().orc_decode_stream_seeded(ch, bs, ptr(rows, u8p), slot, m, ptr(op, f32p), ptr(ob, i32p), C.byref(sd))
    alive = 0
    while alive < m and 0 < ob[alive] <= 8 * ext[alive]:    # (the oracle itself stops at its first block of 0 bits)
        alive += 1
    warm = first - k0                                       # 1: row 0 of the oracle's run is the block in front
    live = max(0, alive - warm)
    pcm[:live] = op.reshape(m, bs, ch)[warm:warm + live]
    bits[:live] = ob[warm:warm + live]
    return pcm, bits, live


def expected_crop_row(payload, offs, rng_states, ch, bs, first, n, count=None, pcm16=False):
    """Row (file, first[, count]) of a block crop -> (pcm [n][bs][ch], bits [n]): the model's leading count blocks, zeros behind."""
    m = n if count is None else max(0, min(n, int(count)))
    pcm, bits = np.zeros((n, bs, ch), np.float32), np.zeros(n, np.int32)
    if m > 0:
        pcm[:m], bits[:m], _ = local_model(payload, offs, rng_states, ch, bs, first, m)
    return (to_pcm16(pcm) if pcm16 else pcm), bits


def expected_sample_row(payload, offs, rng_states, ch, bs, start, n_samples, length=None, pcm16=False):
    """Row (file, start[, length]) of a sample crop -> (pcm [ch][n_samples], bits [blocks_of(bs, n_samples)]): the model's stream
    sliced at the sample, channels-first; zeros behind the length, behind the file's end and from the dead block on; the sizes
    of the blocks the row touches, 0 behind them (as test_gpu_sample_crops.expected_row on a clean file)."""
    K = len(offs) - 1
    nB = blocks_of(bs, n_samples)
    out, bits = np.zeros((ch, n_samples), np.float32), np.zeros(nB, np.int32)
    ln = n_samples if length is None else max(0, min(n_samples, int(length)))
    if start >= 0 and start // bs <= K and ln > 0:
        first, skip = start // bs, start % bs
        m = (start + ln - 1) // bs - first + 1              # blocks the row touches
        pcm, mb, _ = local_model(payload, offs, rng_states, ch, bs, first, m)
        stream = pcm.reshape(m * bs, ch).T
        out[:, :ln] = stream[:, skip:skip + ln]
        bits[:m] = mb
    return (to_pcm16(out) if pcm16 else out), bits


# ---------------------------------------------------------------------------------------------------------------------
# damages
# ---------------------------------------------------------------------------------------------------------------------
def damage_block(payload, offs, k, seed):
    """A copy of the payload with ONE nybble of block k overwritten by another value, at a seeded position anywhere in the
    block's extent (seek_testlib.damaged, confined to the block)."""
    rng = np.random.default_rng(seed)
    a, b = int(offs[k]), int(offs[k + 1])
    q = 2 * a + int(rng.integers(0, 2 * (b - a)))           # nybble number within the payload
    out = payload.copy()
    sh = 4 * (q & 1)
    old = (int(out[q >> 1]) >> sh) & 15
    new = (old + int(rng.integers(1, 16))) & 15
    out[q >> 1] = (int(out[q >> 1]) & ~(15 << sh)) | (new << sh)
    return out


def classify(payload, offs, rng_states, ch, bs, k, seed):
    """What damage_block(payload, offs, k, seed) does to the row that starts with block k, by the model: 'kill' (the row ends at
    k), 'resize' (the block's size changes, the row lives), 'value' / 'draws' (samples change, no size does, nothing dies; 'draws':
    block k + 2, which no lapping of block k reaches, changes too - the block draws another number of noise values and the
    generator is displaced behind it) or 'none' (a nybble behind the block's last bit)."""
    n = min(3, len(offs) - 1 - k)
    cp, cb, cl = local_model(payload, offs, rng_states, ch, bs, k, n)
    p, b, live = local_model(damage_block(payload, offs, k, seed), offs, rng_states, ch, bs, k, n)
    assert cl == n and live in (0, n), (k, seed, cl, live)  # (the blocks behind k are clean: they parse whatever state they meet)
    if live == 0:
        return "kill"
    if not np.array_equal(b, cb):
        return "resize"
    ch_ = [not same_bytes(p[i], cp[i]) for i in range(n)]
    if not any(ch_):
        return "none"
    if n < 3 or not (ch_[0] and ch_[1]):
        return "other"                                      # (a late sub-block's samples leave with the next block; an early one's lap nowhere)
    return "draws" if ch_[2] else "value"


def first_seed(payload, offs, rng_states, ch, bs, k, classes, cache=None):
    """The first seed below MAX_SEED whose damage of block k is of one of `classes`, or None."""
    cache = {} if cache is None else cache
    for sd in range(MAX_SEED):
        if (k, sd) not in cache:
            cache[(k, sd)] = classify(payload, offs, rng_states, ch, bs, k, sd)
        if cache[(k, sd)] in classes:
            return sd
    return None


def fill_block(payload, offs, k):
    """The 0x11 fill of bytes 2 .. 40 of block k (tests/test_gpu_parity.py): long zero runs that overrun any unit."""
    out = payload.copy()
    a, b = int(offs[k]), int(offs[k + 1])
    out[a + 2:min(a + 40, b)] = 0x11
    return out


def kill_block(payload, offs, k, rng_states, ch, bs, cache=None):
    """-> (payload copy, seed or None): the first seed below MAX_SEED for which the model ends the row at block k; the 0x11 fill
    where there is none."""
    sd = first_seed(payload, offs, rng_states, ch, bs, k, ("kill",), cache)
    return (damage_block(payload, offs, k, sd), sd) if sd is not None else (fill_block(payload, offs, k), None)


def value_block(payload, offs, k, rng_states, ch, bs, cache=None):
    """-> (payload copy, seed): the first seed that changes samples - of block k and of block k + 1 -, changes no size and kills nothing."""
    sd = first_seed(payload, offs, rng_states, ch, bs, k, ("value", "draws"), cache)
    assert sd is not None, f"no seed below {MAX_SEED} changes only values of block {k}"
    return damage_block(payload, offs, k, sd), sd


def resize_block(payload, offs, k, rng_states, ch, bs, cache=None):
    """-> (payload copy, seed), or (None, None): the first seed, if any below MAX_SEED, that changes a size and leaves the row alive."""
    sd = first_seed(payload, offs, rng_states, ch, bs, k, ("resize",), cache)
    return (damage_block(payload, offs, k, sd), sd) if sd is not None else (None, None)


def draws_block(payload, offs, k, rng_states, ch, bs, cache=None):
    """-> (payload copy, seed), or (None, None): the first value damage that also changes the block's draw count."""
    sd = first_seed(payload, offs, rng_states, ch, bs, k, ("draws",), cache)
    return (damage_block(payload, offs, k, sd), sd) if sd is not None else (None, None)


class Stream(File):
    """A clean corpus_testlib.File - payload, offs, seeds, wc: its oracle index - with the model and the damages bound to that
    index.  It shares the File's state, so what either computes of the oracle is computed once."""

    def __init__(self, f):
        self.__dict__ = f.__dict__
        self.__dict__.setdefault("_cls", {})

    def model(self, payload, first, n):
        return local_model(payload, self.offs, self.seeds, self.ch, self.bs, first, n)

    def damage(self, kind, k):
        """kind 'kill' / 'value' / 'draws' / 'resize' of block k -> (payload copy or None, seed or None); the seed scans are shared."""
        fn = {"kill": kill_block, "value": value_block, "draws": draws_block, "resize": resize_block}[kind]
        return fn(self.payload, self.offs, k, self.seeds, self.ch, self.bs, self._cls)


# ---------------------------------------------------------------------------------------------------------------------
# corpora
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_of(geom):
    """The geometry's clean stream: the first of seek_testlib.geometries(), or the local 1024 x 2 one."""
    bs, ch = geom
    if geom in EXTRA:
        return Stream(oracle_file(bs, ch, *EXTRA[geom]))
    return Stream(geom_files(geom)[0])


def switched_position(st):
    """A window-switched block (WindowCtrl other than 0x10) away from POSITIONS and from both ends, or None."""
    sw = [k for k in range(st.K) if int(st.wc[k]) != 0x10]
    far = [k for k in sw if 10 <= k <= st.K - 6]
    near = [k for k in sw if 2 <= k <= st.K - 6 and k not in POSITIONS]
    return far[0] if far else near[0] if near else None


class DamagedCorpus:
    """Files of one geometry that share the clean stream's index: copies of its payload, each with one damaged block.
    files[f] = (kind, position or None, seed or None); every payload has the clean one's byte count.  layout: both layouts
    (corpus_testlib.Corpus of F times the clean file, with these payloads), whose arrays read as this object's own."""

    def __init__(self, st, specs, clean=True):
        """specs: [(kind, position)]; a resize that no seed gives is left out.  clean: file 0 is the undamaged payload."""
        self.st, self.bs, self.ch, self.K = st, st.bs, st.ch, st.K
        self.files, self.payloads = ([("clean", None, None)], [st.payload]) if clean else ([], [])
        for kind, j in specs:
            if kind == "value?":                             # a value damage - one that moves the generator, where a seed gives one -; the intact payload where the block takes none
                sd = first_seed(st.payload, st.offs, st.seeds, st.ch, st.bs, j, ("draws",), st._cls)
                sd = first_seed(st.payload, st.offs, st.seeds, st.ch, st.bs, j, ("value",), st._cls) if sd is None else sd
                kind, pay = ("value", damage_block(st.payload, st.offs, j, sd)) if sd is not None else ("intact", st.payload)
            else:
                pay, sd = st.damage(kind, j)
            if pay is not None:
                assert pay.shape == st.payload.shape and (kind == "intact") == np.array_equal(pay, st.payload)
                self.files.append((kind, j, sd)); self.payloads.append(pay)
        self.F = len(self.files)
        self.layout = Corpus([st] * self.F, payloads=self.payloads)
        self._rows = {}

    def __getattr__(self, name):
        if name == "layout":
            raise AttributeError(name)
        return getattr(self.layout, name)                       # host / nbytes / index / count / rpay / poffs / ridx / ioffs / to_device()

    def of_kind(self, kind, j=None):
        return [f for f, (kd, pos, _) in enumerate(self.files) if kd == kind and (j is None or pos == j)]

    def model(self, f, first, n):
        key = (f, int(first), n)
        if key not in self._rows:
            self._rows[key] = self.st.model(self.payloads[f], int(first), n)
        return self._rows[key]

    def crop_row(self, f, first, n, count=None, pcm16=False):
        return expected_crop_row(self.payloads[f], self.st.offs, self.st.seeds, self.ch, self.bs, int(first), n, count, pcm16)

    def sample_row(self, f, start, n_samples, length=None, pcm16=False):
        return expected_sample_row(self.payloads[f], self.st.offs, self.st.seeds, self.ch, self.bs, int(start), n_samples, length, pcm16)


@functools.lru_cache(maxsize=None)
def geometry_corpus(geom):
    st = stream_of(geom)
    return DamagedCorpus(st, [(kind, j) for j in positions_of(geom) for kind in KINDS])


def positions_of(geom):
    """The damaged blocks of a geometry's corpus: POSITIONS and one window-switched block."""
    jw = switched_position(stream_of(geom))
    return POSITIONS + ((jw,) if jw is not None else ())


SWEEP_GEOM, SWEEP_FILES = (2048, 2), 31


@functools.lru_cache(maxsize=None)
def sweep_corpus(kind):
    """31 copies of the 40-block stereo 2048 payload, file j damaged (kill / value) at block j.  (No nybble of a block of pure
    silence gives a value damage: such a file of the value set stays intact.)"""
    return DamagedCorpus(stream_of(SWEEP_GEOM), [("value?" if kind == "value" else kind, j) for j in range(SWEEP_FILES)], clean=False)


RELS = (-4, -3, -2, 0, 1, 2)                                # a row of 4 blocks from block j + rel: the damage at j lies behind the row,
REL_NAMES = ("behind the row", "last", "middle", "first", "warm block", "in front of the warm block")   # is its last block, ...


def rows_around(j, n=4):
    """(first, place) of the n-block rows that put block j in every place of a row."""
    assert n == 4
    return [(j + r, nm) for r, nm in zip(RELS, REL_NAMES)]
