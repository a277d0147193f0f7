"""The call axis: every call family behind every call family on ONE encoder and ONE decoder object.

An object is not stateless between families: it builds, grows and swaps things lazily, and the families share them (DESIGN.md,
"Call classes").  This library holds the model that says what every call of a designed sequence must write, from the oracle
alone, whatever ran on the object before:

  the lives model   _Slots and the cached oracle helpers of tests/test_gpu_slots.py (moved here, imported back there): a slot's life
                    is the oracle's uninterrupted run of what the slot was fed, across every call it took part in and every call
                    it did not; resets, saves / loads (into another slot too), range calls and uploads start lives.
  families          one class per call family: plan() chooses a call's parameters from the model's state, apply() advances the
                    model and returns (inputs, expected outputs) as numpy, call() makes the device call.  FAMILIES is the table.
  sequence()        a deterministic list of calls in which every ordered pair of families of an object occurs as consecutive
                    calls (an Eulerian circuit of the complete digraph with self-loops), prepared once per process.
  run()             a sequence against a backend - the library on a GPU (GpuBackend) or a stand-in made of the model itself
                    (StandIn, tests/test_call_axis_capi.py) - with every output of every call compared bit for bit.

Corpus-side references come from the existing models (corpus_testlib.File / Corpus, lowrate_testlib, clips_testlib,
clips_ladder_testlib, clip_spectra_testlib); nothing here restates the codec.  CPU only, except GpuBackend (torch and the library
are imported when it is made)."""
import copy
import functools
import numpy as np

from ulc_testlib import synth_pcm, oracle_encode_debug, oracle_decode_stream, to_pcm16
from rates_testlib import mode_of

RATE = 44100
N_BLOCKS = 48                                              # PCM / oracle blocks per test stream of tests/test_gpu_slots.py
VBR50, CBR64 = (-50.0, 0.0), (64.0, 0.0)                   # settings in the tool's convention (rates_testlib.mode_of)
TABLE = [(-50.0, 0.0), (64.0, 0.0), (96.0, 0.3), (-70.0, 0.0), (48.0, 0.0)]      # per-stream table: VBR / CBR / ABR by stream id
BIG = (2048, 2, 70, 8)                                     # (BlockSize, channels, slots, maxBlocksPerCall): the fused window control, k_select_wave
SMALL = (512, 1, 9, 8)                                     # generic selection, non-fused window control


# ---------------------------------------------------------------------------------------------------------------------
# the lives model of tests/test_gpu_slots.py: inputs and oracle references, computed once
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pcm(bs, ch, sid):
    """[N_BLOCKS][bs][ch]; every third stream is transient-rich, so that decimated windows occur"""
    return synth_pcm(sid, N_BLOCKS * bs, ch, RATE, transient=(sid % 3 == 0), seed=bs + ch).reshape(N_BLOCKS, bs, ch)


@functools.lru_cache(maxsize=None)
def _oracle_enc(bs, ch, sid, origin, n, setting):
    """The oracle's encode of blocks origin .. origin + n - 1 of stream sid's PCM from a fresh state, under one setting."""
    mode, p0, p1 = mode_of(setting)
    return oracle_encode_debug(_pcm(bs, ch, sid)[origin:origin + n].reshape(n * bs, ch), bs, RATE, mode, p0, p1, slot=2 * ch * bs + 16)


@functools.lru_cache(maxsize=None)
def _oracle_blocks(bs, ch, sid):
    """Oracle-encoded VBR 50 blocks of stream sid: (blocks [N_BLOCKS][slot], bits)"""
    r = _oracle_enc(bs, ch, sid, 0, N_BLOCKS, VBR50)
    return r["out"], r["bits"]


@functools.lru_cache(maxsize=None)
def _oracle_dec(bs, ch, key):
    """The oracle's decode from a fresh state of the blocks `key` names: ((sid, first block, count), ...) concatenated."""
    blocks = np.concatenate([_oracle_blocks(bs, ch, sid)[0][a:a + n] for sid, a, n in key])
    rc, pcm, bits = oracle_decode_stream(blocks, ch, bs)
    assert rc == 0
    return pcm.reshape(len(blocks), bs, ch), bits


def _setting_fn(what):
    return (lambda sid: TABLE[sid % len(TABLE)]) if what == "table" else (lambda sid: what)


class _Slots:
    def __init__(self, geom, sid=None):
        self.bs, self.ch, self.B, self.maxK = geom
        self.sid = list(range(self.B)) if sid is None else list(sid)          # the test stream that feeds each slot
        self.pos = [0] * self.B                                               # next block of it
        self.lives = [[dict(sid=self.sid[s], origin=0, first=0, blocks=[])] for s in range(self.B)]

    def new_life(self, slot, sid=None, origin=None, first=0):
        """slot starts another stream (a reset: the same PCM from where it stands) or takes one over (a load: first blocks done elsewhere)"""
        if sid is not None:
            self.sid[slot] = sid
        if origin is not None:
            self.pos[slot] = origin + first
        self.lives[slot].append(dict(sid=self.sid[slot], origin=self.pos[slot] - first, first=first, blocks=[]))

    def rows(self, slots, K, bad):
        """(sid, first block) per row; a list entry outside [0, B) is fed stream bad[row] from its block 0"""
        r = []
        for i, s in enumerate(slots):
            ok = 0 <= s < self.B
            r.append((self.sid[s], self.pos[s]) if ok else (bad[i], 0))
            assert r[-1][1] + K <= N_BLOCKS
        return r

    def keep(self, slots, K, per_row):
        """per_row[i][k] -> the slot's current life; rows of entries outside [0, B) are returned"""
        extra = {}
        for i, s in enumerate(slots):
            if 0 <= s < self.B:
                self.lives[s][-1]["blocks"] += per_row[i]
                self.pos[s] += K
            else:
                extra[i] = per_row[i]
        return extra


# ---------------------------------------------------------------------------------------------------------------------
# the call axis: streams, and the references every family shares
# ---------------------------------------------------------------------------------------------------------------------
DEC_GEOMS = {"2048x2x6": (2048, 2, 6, 24),                 # k_dsyn with two state sets: long rows take the even cut
             "512x1x9": (512, 1, 9, 8)}                    # k_dgen: one set, never cut
ENC_GEOMS = {"2048x2x70": (2048, 2, 70, 8),                # across the 64-stream group of the window-control kernels
             "512x1x9": (512, 1, 9, 8)}
GEOMS = {"dec": DEC_GEOMS, "enc": ENC_GEOMS}
STARTS = ("a", "b")                                        # a: the walk from a streaming call; b: every lazy piece built in front of it
DEC_BLOCKS, ENC_BLOCKS = 160, 64                           # blocks of a decoder / an encoder test stream of the axis
RESIDENT_WG = 1536                                         # k_dsyn workgroups an MI355X holds for stereo 2048 (include/ulc_amd.h): the census's cut
POISON = 0xA5
LADDER2 = (VBR50, "table")
LADDER4 = (VBR50, CBR64, "table", CBR64)                   # (a rung must not depend on its place: CBR 64 twice)


@functools.lru_cache(maxsize=None)
def ax_pcm(bs, ch, sid, n):
    """[n][bs][ch] on the PCM16 grid; every third stream is transient-rich"""
    return synth_pcm(sid, n * bs, ch, RATE, transient=(sid % 3 == 0), seed=bs + ch).reshape(n, bs, ch)


@functools.lru_cache(maxsize=None)
def enc_ref(bs, ch, sid, setting):
    """The oracle's encode of stream sid's ENC_BLOCKS blocks from a fresh state under one setting (an encoder slot's state is
    the blocks it has consumed of its stream: the setting of a block changes no state, tests/test_gpu_ladder.py)."""
    mode, p0, p1 = mode_of(setting)
    return oracle_encode_debug(ax_pcm(bs, ch, sid, ENC_BLOCKS).reshape(ENC_BLOCKS * bs, ch), bs, RATE, mode, p0, p1, slot=2 * ch * bs + 16)


@functools.lru_cache(maxsize=None)
def dec_file(bs, ch, sid):
    """Stream sid of a decoder sequence as a corpus_testlib.File: DEC_BLOCKS oracle-encoded VBR 50 blocks."""
    from corpus_testlib import File
    r = oracle_encode_debug(ax_pcm(bs, ch, sid, DEC_BLOCKS).reshape(DEC_BLOCKS * bs, ch), bs, RATE, 0, 50.0, 0.0, slot=2 * ch * bs + 16)
    return File(f"axis stream {sid} {bs}x{ch}", bs, ch, r["out"], r["bits"])


_DECODED = {}


def decode_key(bs, ch, key):
    """The oracle's decode from a fresh state of the blocks `key` = ((sid, first, count), ...) -> (pcm [n][bs][ch], bits [n]);
    the last few keys are kept (a life is asked for again while it grows)."""
    k = (bs, ch, key)
    if k not in _DECODED:
        if len(_DECODED) > 64:
            _DECODED.pop(next(iter(_DECODED)))
        blocks = np.concatenate([dec_file(bs, ch, sid).blocks[a:a + n] for sid, a, n in key])
        rc, pcm, bits = oracle_decode_stream(blocks, ch, bs)
        assert rc == 0
        _DECODED[k] = (pcm.reshape(len(blocks), bs, ch), bits)
    return _DECODED[k]


@functools.lru_cache(maxsize=None)
def low_corpus(bs, ch, lgD):
    """lowrate_testlib.LowCase of a geometry at any ratio: the geometry's shared files and, last, a copy of file 0 with one dead
    block under the clean index.  The corpus of every stateless decoder family (the killed file only in the low-rate rows, whose
    model knows it)."""
    import lowrate_testlib as L
    import damage_testlib as D
    from corpus_testlib import Corpus, geom_files
    c = L.LowCase.__new__(L.LowCase)
    c.name, c.bs, c.ch, c.lgD, c.bsr = f"axis {bs}x{ch}/{1 << lgD}", bs, ch, lgD, bs >> lgD
    files = list(geom_files((bs, ch)))
    c.dead_at = min(L.DEAD_AT, files[0].K - 2)
    c.killed, c.kill_seed = D.Stream(files[0]).damage("kill", c.dead_at)
    c.cor = Corpus(files + [files[0]], payloads=[f.payload for f in files] + [c.killed])
    c.dead = [None] * len(files) + [c.dead_at]
    return c


def corpus(bs, ch):
    return low_corpus(bs, ch, 1).cor


def sample_row(cor, f, start, n_samples, length):
    """A sample-crop row (tests/test_gpu_sample_crops.py, expected_row): the file's decoded stream sliced at the sample, zeros
    behind the length and the file's end; the sizes of the blocks the row touches."""
    bs, ch = cor.bs, cor.ch
    out, bits = np.zeros((ch, n_samples), np.float32), np.zeros(1 + (n_samples + bs - 2) // bs, np.int32)
    ln = max(0, min(n_samples, int(length)))
    if 0 <= f < cor.F and start >= 0 and start // bs <= cor.K[f] and ln > 0:
        stream = cor.files[f].pcm.reshape(cor.K[f] * bs, ch).T
        end = min(start + ln, cor.K[f] * bs)
        if end > start:
            out[:, :end - start] = stream[:, start:end]
        for b in range(start // bs, (start + ln - 1) // bs + 1):
            if b < cor.K[f]:
                bits[b - start // bs] = cor.files[f].obits[b]
    return out, bits


def predicted_cut(bs, ch, n, K):
    """Workgroups of the even cut the decoder plans for K blocks of n streams on an MI355X (0: none; host arithmetic of the library)."""
    if (bs, ch) != (2048, 2):
        return 0
    from gpu_testlib import amd
    return int(amd().lib().ulcx_dec_split_plan(int(n), int(K), RESIDENT_WG))


# ---------------------------------------------------------------------------------------------------------------------
# the models: what an object holds between calls, as far as any call can tell
# ---------------------------------------------------------------------------------------------------------------------
class DecModel(_Slots):
    """A decoder slot is what it was fed since its life began - key, the ((stream, first block, count), ...) of it - and where the
    library's packed read position stands (ppos, in blocks of the slot's stream).  pos is the test's own cursor: the block a
    slot-form call feeds next."""
    kind, stream_blocks = "dec", DEC_BLOCKS

    def __init__(self, geom):
        super().__init__(geom)
        self.key = [() for _ in range(self.B)]
        self.ppos = [0] * self.B
        self.n_lives = [1] * self.B
        self.records = {}                                   # record id -> [snapshot per listed slot]
        self.resident = None                                # stream ids of the uploaded payload; has_index
        self.host_slot = 0                                  # largest slotBytes a host-form call brought

    def file(self, s):
        return dec_file(self.bs, self.ch, self.sid[s])

    def feed(self, s, a, K):
        """slot s decodes blocks a .. a + K - 1 of its stream -> (pcm [K][bs][ch], bits [K]) the oracle gives for them"""
        assert a + K <= DEC_BLOCKS, f"slot {s}: block {a} + {K} of a stream of {DEC_BLOCKS}"
        key = self.key[s]
        if key and key[-1][0] == self.sid[s] and key[-1][1] + key[-1][2] == a:
            key = key[:-1] + ((self.sid[s], key[-1][1], key[-1][2] + K),)
        else:
            key = key + ((self.sid[s], a, K),)
        self.key[s] = key
        pcm, bits = decode_key(self.bs, self.ch, key)
        return pcm[-K:], bits[-K:]

    def fresh(self, s):
        self.key[s], self.pos[s], self.ppos[s] = (), 0, 0
        self.n_lives[s] += 1

    def snapshot(self, s):
        return dict(sid=self.sid[s], key=self.key[s], pos=self.pos[s], ppos=self.ppos[s])

    def restore(self, s, snap):
        self.sid[s], self.key[s], self.pos[s], self.ppos[s] = snap["sid"], snap["key"], snap["pos"], snap["ppos"]
        self.n_lives[s] += 1

    def state(self):
        """what save_streams of all slots holds, as far as the model knows it"""
        return [(self.key[s], self.ppos[s]) for s in range(self.B)]

    def room(self, s):
        return DEC_BLOCKS - max(self.pos[s], self.ppos[s])


class EncModel(_Slots):
    """An encoder slot is the blocks it has consumed of its stream (pos): every life starts at block 0 of a stream."""
    kind, stream_blocks = "enc", ENC_BLOCKS

    def __init__(self, geom):
        super().__init__(geom)
        self.n_lives = [1] * self.B
        self.records = {}
        self.lad_rungs = 0                                  # rungs of the widest host ladder call so far (ladOut / ladRungs)
        self.clip_rungs = 0                                 # rungs of the widest clips call so far (clips_staging)

    def feed(self, s, K, setting, pcm16=False):
        """-> (out [K][slot], bits [K], wc [K], cplx [K]) of the slot's next K blocks under `setting`"""
        a = self.pos[s]
        assert a + K <= ENC_BLOCKS, f"slot {s}: block {a} + {K} of a stream of {ENC_BLOCKS}"
        r = enc_ref(self.bs, self.ch, self.sid[s], tuple(setting))
        self.pos[s] = a + K
        return r["out"][a:a + K], r["bits"][a:a + K], r["wc"][a:a + K], r["cplx"][a:a + K]

    def pcm_in(self, s, K):
        return ax_pcm(self.bs, self.ch, self.sid[s], ENC_BLOCKS)[self.pos[s]:self.pos[s] + K]

    def fresh(self, s):
        self.pos[s] = 0
        self.n_lives[s] += 1

    def snapshot(self, s):
        return dict(sid=self.sid[s], pos=self.pos[s])

    def restore(self, s, snap):
        self.sid[s], self.pos[s] = snap["sid"], snap["pos"]
        self.n_lives[s] += 1

    def state(self):
        return [(self.sid[s], self.pos[s]) for s in range(self.B)]

    def room(self, s):
        return ENC_BLOCKS - self.pos[s]

    def setting(self, s):
        return TABLE[self.sid[s] % len(TABLE)]


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
class Op:
    """One call of a sequence: its family and the parameters plan() chose.  first: the first call of its family on the object."""

    def __init__(self, i, family, prev, first, hint):
        self.i, self.family, self.prev, self.first, self.hint, self.p = i, family, prev, first, hint, {}

    def __repr__(self):
        return f"op {self.i} ({self.prev or 'create'} -> {self.family}{', the first ' + self.family + ' call of the object' if self.first else ''}) {self.p}"


class Family:
    """plan(m, op, rng): parameters into op.p from the model's state.  apply(m, op) -> (inputs, expected): numpy arrays by name; an
    expected entry may be (array, mask) - only the elements under the mask are defined.  call(obj, op, P, stream, aux): the device
    call, P(name) the device address of an input or output (host forms: call(obj, op, inputs) -> outputs).
    streaming: reads or advances stream state.  host: a host-pointer form (synchronous; not part of the unsynchronised chain).
    exports: the entries of the binding's signature tables the family calls.  lazy(m, op): [(piece, level)] the call needs."""
    name = kind = None
    streaming = True
    host = False
    exports = ()
    cuts = False                                            # the call's synthesis can take the even cut

    def lazy(self, m, op):
        return []

    def outs(self, expected):
        return {k: ((v[0] if isinstance(v, tuple) else v).shape, (v[0] if isinstance(v, tuple) else v).dtype) for k, v in expected.items()}


def _slot_list(m, rng, n, need):
    """n slots in a seeded order, those with the most room first among equals; every one has room for `need` blocks"""
    order = [int(s) for s in rng.permutation(m.B) if m.room(int(s)) >= need]
    assert order, "no slot has room: the sequence needs longer streams or more resets"
    return np.array(order[:max(1, min(n, len(order)))], np.int32)


def _K_all(m, want):
    """the call's K, clipped to what every slot still has of its stream"""
    room = min(m.room(s) for s in range(m.B))
    assert room >= 1, "a slot is at the end of its stream: the sequence needs longer streams or more resets"
    if m.kind == "dec" and not any(m.key):
        want = max(want, 2)                                 # (a stream's block 0 decodes to silence: no call of that alone)
    return min(want, room)


# ---- decoder, streaming ---------------------------------------------------------------------------------------------
class DecPlain(Family):
    kind, name, exports, cuts = "dec", "decode", ("ulcx_decode_dev",), True
    pcm16 = False

    def plan(self, m, op, rng):
        op.p.update(K=_K_all(m, op.hint["K"]))

    def apply(self, m, op):
        K = op.p["K"]
        x = np.stack([m.file(s).blocks[m.pos[s]:m.pos[s] + K] for s in range(m.B)])
        rows = [m.feed(s, m.pos[s], K) for s in range(m.B)]
        for s in range(m.B):
            m.pos[s] += K
        pcm = np.stack([r[0] for r in rows])
        return dict(d_in=x), dict(pcm=to_pcm16(pcm) if self.pcm16 else pcm, bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, P, stream, aux):
        fn = obj.decode_dev_pcm16 if self.pcm16 else obj.decode_dev
        fn(P("d_in"), 2 * obj.C * obj.BS + 16, op.p["K"], P("pcm"), P("bits"), stream=stream)


class DecPlain16(DecPlain):
    name, exports, pcm16 = "decode_pcm16", ("ulcx_decode_dev_pcm16",), True


class DecSubset(Family):
    kind, name, exports, cuts = "dec", "decode_subset", ("ulcx_decode_dev_subset",), True
    pcm16 = False

    def lazy(self, m, op):
        return [("dec_shadow", 1)]

    def plan(self, m, op, rng):
        slots = _slot_list(m, rng, op.hint["n"], 1)
        K = max(op.hint["K"], 1 if any(m.key[int(s)] for s in slots) else 2)
        op.p.update(slots=slots, K=max(1, min(K, min(m.room(int(s)) for s in slots))))

    def apply(self, m, op):
        K, slots = op.p["K"], [int(s) for s in op.p["slots"]]
        x = np.stack([m.file(s).blocks[m.pos[s]:m.pos[s] + K] for s in slots])
        rows = [m.feed(s, m.pos[s], K) for s in slots]
        for s in slots:
            m.pos[s] += K
        pcm = np.stack([r[0] for r in rows])
        return dict(slots=op.p["slots"], d_in=x), dict(pcm=to_pcm16(pcm) if self.pcm16 else pcm, bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, P, stream, aux):
        obj.decode_subset_dev(P("slots"), len(op.p["slots"]), P("d_in"), 2 * obj.C * obj.BS + 16, op.p["K"], P("pcm"), P("bits"), stream=stream, pcm16=self.pcm16)


class DecSubset16(DecSubset):
    name, exports, pcm16 = "decode_subset_pcm16", ("ulcx_decode_dev_pcm16_subset",), True


def _payloads(m):
    """the packed payloads of the slots' streams, one row per slot: (payload [B][stride], bytes [B]); the stride is one for all streams"""
    files = [m.file(s) for s in range(m.B)]
    stride = (max(dec_file(m.bs, m.ch, sid).payload.size for sid in range(m.B)) + 64 + 15) & ~15
    host = np.zeros((m.B, stride), np.uint8)
    for s, f in enumerate(files):
        host[s, :f.payload.size] = f.payload
    return host, np.array([f.payload.size for f in files], np.int32)


class DecPacked(Family):
    kind, name, exports, cuts = "dec", "decode_packed", ("ulcx_decode_packed_dev",), True

    def plan(self, m, op, rng):
        op.p.update(K=_K_all(m, op.hint["K"]))

    def apply(self, m, op):
        K = op.p["K"]
        pay, nb = _payloads(m)
        rows = [m.feed(s, m.ppos[s], K) for s in range(m.B)]
        for s in range(m.B):
            m.ppos[s] += K
            m.pos[s] = m.ppos[s]                            # the slot-form calls go on behind the packed ones
        return dict(payload=pay, nbytes=nb), dict(pcm=np.stack([r[0] for r in rows]), bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, P, stream, aux):
        obj.decode_packed_dev(P("payload"), aux["payload"].shape[1], P("nbytes"), op.p["K"], P("pcm"), P("bits"), stream=stream)


def _index_of(m, cap):
    idx = np.stack([m.file(s).row(cap) for s in range(m.B)])
    return idx, np.full(m.B, DEC_BLOCKS, np.int32)


def _range_model(m, first, K):
    """a range call's rows and the lives it starts: every slot is then a sequential decode of its stream up to the range's end"""
    pcm, bits = [], []
    for s in range(m.B):
        f = int(first[s])
        p, b = m.file(s).expected_pcm(f, K)
        pcm.append(p); bits.append(b)
        m.key[s] = ((m.sid[s], 0, f + K),)
        m.pos[s] = m.ppos[s] = f + K
        m.n_lives[s] += 1
    return np.stack(pcm), np.stack(bits)


class DecRange(Family):
    kind, name, exports, cuts = "dec", "decode_range", ("ulcx_decode_range_dev", "ulcx_decode_range_dev_pcm16"), True

    def plan(self, m, op, rng):
        K = max(1, min(op.hint["K"], m.maxK - 1))
        op.p.update(K=K, first=rng.integers(0, 12, m.B).astype(np.int32), pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        pay, nb = _payloads(m)
        idx, cnt = _index_of(m, DEC_BLOCKS + 1)
        pcm, bits = _range_model(m, op.p["first"], op.p["K"])
        return dict(payload=pay, nbytes=nb, index=idx, count=cnt, first=op.p["first"]), dict(pcm=to_pcm16(pcm) if op.p["pcm16"] else pcm, bits=bits)

    def call(self, obj, op, P, stream, aux):
        obj.decode_range_dev(P("payload"), aux["payload"].shape[1], P("nbytes"), P("index"), DEC_BLOCKS + 1, P("count"), P("first"), op.p["K"],
                             P("pcm"), P("bits"), stream=stream, pcm16=op.p["pcm16"])


class DecResident(Family):
    """The resident path, host forms.  Step 0: upload_payload (a whole-object reset: every slot starts a life), index_resident, a
    range from the kept index.  Step 1: decode_resident, the packed call on the resident copy.  Step 2: set_resident_index (a
    stored index in place of the walk) and a range from it."""
    kind, name, host, cuts = "dec", "resident", True, True
    exports = ("ulcx_decoder_upload_payload", "ulcx_decoder_index_resident", "ulcx_decode_resident_range_host", "ulcx_decoder_set_resident_index",
               "ulcx_decode_resident_host")

    def lazy(self, m, op):
        return [("resident_payload", 1), ("resident_index", 1)] if op.p["step"] == 0 else [("dec_host_out", 1)]

    def plan(self, m, op, rng):
        step = op.hint["j"] % 3 if m.resident is not None and m.resident == m.sid else 0
        K = max(1, min(op.hint["K"], m.maxK - 1))
        if step == 1:
            K = _K_all(m, K)
        op.p.update(step=step, K=K, first=rng.integers(0, 12, m.B).astype(np.int32))

    def apply(self, m, op):
        step, K = op.p["step"], op.p["K"]
        pay, nb = _payloads(m)
        idx, cnt = _index_of(m, DEC_BLOCKS + 1)
        exp = {}
        if step == 0:
            for s in range(m.B):
                m.fresh(s)
            m.resident = list(m.sid)
            exp["count"] = cnt
        if step == 1:
            rows = [m.feed(s, m.ppos[s], K) for s in range(m.B)]
            for s in range(m.B):
                m.ppos[s] += K
                m.pos[s] = m.ppos[s]
            exp.update(pcm=np.stack([r[0] for r in rows]), bits=np.stack([r[1] for r in rows]))
        else:
            exp["pcm"], exp["bits"] = _range_model(m, op.p["first"], K)
        return dict(payload=pay, nbytes=nb, index=idx, count=cnt, first=op.p["first"]), exp

    def call(self, obj, op, inp):
        step, K, out = op.p["step"], op.p["K"], {}
        if step == 0:
            obj.upload_payload(inp["payload"], inp["nbytes"])
            out["count"] = obj.index_resident(DEC_BLOCKS)
        if step == 2:
            obj.set_resident_index(inp["index"], inp["count"])
        pcm, bits = obj.decode_resident(K) if step == 1 else obj.decode_resident_range(inp["first"], K)
        out.update(pcm=pcm.reshape(obj.B, K, obj.BS, obj.C), bits=bits)
        return out


class DecHost(Family):
    """ulcx_decode_host with a slotBytes that grows once: the first calls bring slots just large enough for their blocks, the
    later ones the full slot - the object regrows its staging."""
    kind, name, host, exports, cuts = "dec", "decode_host", True, ("ulcx_decode_host",), True

    def lazy(self, m, op):
        return [("dec_host_in", 2 if op.p["full"] else 1), ("dec_host_out", 1)]

    def plan(self, m, op, rng):
        op.p.update(K=_K_all(m, op.hint["K"]), full=op.hint["j"] >= 2)

    def apply(self, m, op):
        K = op.p["K"]
        x = np.stack([m.file(s).blocks[m.pos[s]:m.pos[s] + K] for s in range(m.B)])
        if not op.p["full"]:
            x = np.ascontiguousarray(x[:, :, :int(max(m.file(s).nb[m.pos[s]:m.pos[s] + K].max() for s in range(m.B))) + 1])
        m.host_slot = max(m.host_slot, x.shape[2])
        rows = [m.feed(s, m.pos[s], K) for s in range(m.B)]
        for s in range(m.B):
            m.pos[s] += K
        return dict(d_in=x), dict(pcm=np.stack([r[0] for r in rows]), bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, inp):
        pcm, bits = obj.decode(inp["d_in"])
        return dict(pcm=pcm.reshape(obj.B, op.p["K"], obj.BS, obj.C), bits=bits)


class Reset(Family):
    """reset_streams_dev of the slots that are furthest along their streams - every slot past the middle of its stream, and 1, 5
    or half of the slots at the least (they replay their stream from its block 0)."""
    name = "reset_streams"

    def plan(self, m, op, rng):
        order = sorted(range(m.B), key=lambda s: (m.room(s), s))
        n = max(1, min(op.hint["n"], (m.B + 1) // 2), len([s for s in order if 2 * m.room(s) < m.stream_blocks]))
        op.p.update(slots=np.array(order[:n], np.int32))

    def apply(self, m, op):
        for s in op.p["slots"]:
            m.fresh(int(s))
        return dict(slots=op.p["slots"]), {}

    def call(self, obj, op, P, stream, aux):
        obj.reset_streams_dev(P("slots"), len(op.p["slots"]), stream=stream)


class Save(Family):
    """save_streams_dev of a few slots into a record buffer the sequence keeps; the load calls take the latest."""
    name = "save_streams"

    def plan(self, m, op, rng):
        op.p.update(slots=np.array(rng.permutation(m.B)[:max(1, min(op.hint["n"], m.B))], np.int32), rec=op.i)

    def apply(self, m, op):
        m.records[op.p["rec"]] = [m.snapshot(int(s)) for s in op.p["slots"]]
        m.last_record = op.p["rec"]
        if op.hint.get("behind_cut"):
            m.hot_record = op.p["rec"]                      # saved directly behind a cut call: the next load takes this one
        return dict(slots=op.p["slots"]), {}

    def call(self, obj, op, P, stream, aux):
        obj.save_streams_dev(P("slots"), len(op.p["slots"]), P("rec:%d" % op.p["rec"]), stream=stream)


class Load(Family):
    """load_streams_dev of the latest record (first of all, of one saved directly behind a cut call) into other slots than it was saved from (rotated by one); in front of the first
    save, and when slots are past the middle of their streams (into those slots), a record of a fresh object's - which is a reset."""
    name = "load_streams"

    def plan(self, m, op, rng):
        rec = getattr(m, "hot_record", None)
        low = [s for s in range(m.B) if 2 * m.room(s) < m.stream_blocks] if rec is None else []
        rec, m.hot_record = getattr(m, "last_record", None) if rec is None else rec, None
        if rec is None or low:
            op.p.update(rec=None, slots=np.array(low or [m.B - 1], np.int32))
        else:
            n = len(m.records[rec])
            op.p.update(rec=rec, slots=np.array([(int(op.hint["j"]) + 1 + i) % m.B for i in range(n)], np.int32))

    def apply(self, m, op):
        if op.p["rec"] is None:
            fresh = type(m)((m.bs, m.ch, m.B, m.maxK))
            for s in op.p["slots"]:
                snap = fresh.snapshot(0)
                snap["sid"] = m.sid[int(s)]
                m.restore(int(s), snap)
        else:
            for s, snap in zip(op.p["slots"], m.records[op.p["rec"]]):
                m.restore(int(s), copy.deepcopy(snap))
        return dict(slots=op.p["slots"]), {}

    def call(self, obj, op, P, stream, aux):
        obj.load_streams_dev(P("slots"), len(op.p["slots"]), P("rec:%s" % op.p["rec"]), stream=stream)


def _slot_family(base, kind, what):
    return type(f"{kind.title()}{base.__name__}", (base,), dict(kind=kind, name=base.name, exports=(f"ulcx_{what}_{base.name}_dev",)))


# ---- decoder, stateless (no stream's state is read or changed) -------------------------------------------------------------
class _Stateless(Family):
    streaming = False
    kind = "dec"

    def lazy(self, m, op):
        return [("dec_shadow", 1)]

    def corpus_in(self, m):
        c = corpus(m.bs, m.ch)
        return c, dict(payload=c.host, nbytes=c.nbytes, index=c.index, count=c.count)

    def corpus_args(self, c, P):
        return (c.F, P("payload"), c.host.shape[1], P("nbytes"), P("index"), c.istride, P("count"))

    def rows(self, m, rng, n):
        """(file, first block, count) rows over the clean files: seeded starts, a row that runs over its file's end, one that starts
        at the end, one cut short by its count"""
        c = corpus(m.bs, m.ch)
        clean = c.F - 1
        t = [(0, c.K[0] - 1, 9), (clean - 1, c.K[clean - 1], 9), (0, 3, 1)]
        while len(t) < n:
            f = int(rng.integers(0, clean))
            t.append((f, int(rng.integers(0, c.K[f])), 9))
        order = rng.permutation(len(t))[:n]
        return [t[i] for i in order]


class DecCrops(_Stateless):
    name, exports = "decode_crops", ("ulcx_decode_crops_dev", "ulcx_decode_crops_dev_pcm16")

    def plan(self, m, op, rng):
        n = min(op.hint["n8"], m.B)
        op.p.update(rows=self.rows(m, rng, max(n, 3) if m.B >= 3 else n), N=min(op.hint["N3"], m.maxK - 1), pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        c, inp = self.corpus_in(m)
        files, first, count = (np.array(x, np.int32) for x in zip(*op.p["rows"]))
        pcm, bits = c.expected_pcm(files, first, op.p["N"], count)
        inp.update(file=files, first=first, cnt=count)
        return inp, dict(pcm=to_pcm16(pcm) if op.p["pcm16"] else pcm, bits=bits)

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.decode_crops_dev(*self.corpus_args(c, P), len(op.p["rows"]), P("file"), P("first"), P("cnt"), op.p["N"], P("pcm"), P("bits"),
                             stream=stream, pcm16=op.p["pcm16"])


class DecCropsRagged(DecCrops):
    name, exports = "decode_crops_ragged", ("ulcx_decode_crops_ragged_dev", "ulcx_decode_crops_ragged_dev_pcm16")

    def corpus_in(self, m):
        c = corpus(m.bs, m.ch)
        return c, dict(payload=c.rpay, poffs=c.poffs, index=c.ridx, ioffs=c.ioffs, count=c.count)

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.decode_crops_ragged_dev(c.F, P("payload"), c.rpay.size, P("poffs"), P("index"), c.ridx.size, P("ioffs"), P("count"), len(op.p["rows"]),
                                    P("file"), P("first"), P("cnt"), op.p["N"], P("pcm"), P("bits"), stream=stream, pcm16=op.p["pcm16"])


class DecSpectra(DecCrops):
    name, exports = "decode_crops_spectra", ("ulcx_decode_crops_spectra_dev",)

    def apply(self, m, op):
        c, inp = self.corpus_in(m)
        files, first, count = (np.array(x, np.int32) for x in zip(*op.p["rows"]))
        coef, wc, bits = c.expected_spec(files, first, op.p["N"], count, lr=op.p["pcm16"])
        inp.update(file=files, first=first, cnt=count)
        return inp, dict(coef=coef, wc=wc, bits=bits)

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.decode_crops_spectra_dev(*self.corpus_args(c, P), len(op.p["rows"]), P("file"), P("first"), P("cnt"), op.p["N"], 1 if op.p["pcm16"] else 0,
                                     P("coef"), P("wc"), P("bits"), stream=stream)


class DecSamples(_Stateless):
    name, exports = "decode_crops_samples", ("ulcx_decode_crops_samples_dev", "ulcx_decode_crops_samples_dev_pcm16")
    lgD = 0

    def sample_rows(self, m, rng, n, bsr, T):
        c = corpus(m.bs, m.ch)
        clean = c.F - 1
        t = [(0, (c.K[0] - 1) * bsr + 5, T), (0, bsr + bsr // 3 + 1, T), (clean - 1, 2 * bsr + 7, 3)]
        while len(t) < n:
            f = int(rng.integers(0, clean))
            t.append((f, int(rng.integers(0, c.K[f] * bsr)), T))
        return [t[i] for i in rng.permutation(len(t))[:n]]

    def plan(self, m, op, rng):
        bsr = m.bs >> self.lgD
        T = min(op.hint["N3"], m.maxK - 2) * bsr - bsr // 2 + 1            # at most N3 blocks touched, odd
        n = min(op.hint["n8"], m.B)
        op.p.update(rows=self.sample_rows(m, rng, max(n, 3) if m.B >= 3 else n, bsr, T), T=T, pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        c, inp = self.corpus_in(m)
        rows = [sample_row(c, f, st, op.p["T"], ln) for f, st, ln in op.p["rows"]]
        files, start, length = zip(*op.p["rows"])
        inp.update(file=np.array(files, np.int32), start=np.array(start, np.int64), len=np.array(length, np.int32))
        pcm = np.stack([r[0] for r in rows])
        return inp, dict(pcm=to_pcm16(pcm) if op.p["pcm16"] else pcm, bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.decode_crops_samples_dev(*self.corpus_args(c, P), len(op.p["rows"]), P("file"), P("start"), P("len"), op.p["T"], P("pcm"), P("bits"),
                                     stream=stream, pcm16=op.p["pcm16"])


class DecLowrate(DecSamples):
    """Low-rate sample crops at one ratio; the rows include the killed file: one that ends at the dead block and one that starts behind it."""

    def __init__(self, lgD):
        self.lgD, self.name = lgD, f"decode_crops_lowrate/{1 << lgD}"
        self.exports = ("ulcx_decode_crops_lowrate_dev", "ulcx_decode_crops_lowrate_dev_pcm16")

    def lazy(self, m, op):
        return [("dec_shadow", 1), (f"dec_low{self.lgD}", 1)]

    def sample_rows(self, m, rng, n, bsr, T):
        lc = low_corpus(m.bs, m.ch, self.lgD)
        z, d = lc.cor.F - 1, lc.dead_at
        t = super().sample_rows(m, rng, max(1, n - 2), bsr, T)
        return (t + [(z, max(0, (d - 2) * bsr + 9), T), (z, (d + 1) * bsr, T)])[-n:] if n >= 3 else t

    def apply(self, m, op):
        lc = low_corpus(m.bs, m.ch, self.lgD)
        _, inp = self.corpus_in(m)
        inp.update(payload=lc.cor.host)
        rows = [lc.expected_row(f, st, op.p["T"], ln) for f, st, ln in op.p["rows"]]
        files, start, length = zip(*op.p["rows"])
        inp.update(file=np.array(files, np.int32), start=np.array(start, np.int64), len=np.array(length, np.int32))
        pcm = np.stack([r[0] for r in rows])
        return inp, dict(pcm=to_pcm16(pcm) if op.p["pcm16"] else pcm, bits=np.stack([r[1] for r in rows]))

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.decode_crops_lowrate_dev(*self.corpus_args(c, P), len(op.p["rows"]), P("file"), P("start"), P("len"), op.p["T"], self.lgD, P("pcm"),
                                     P("bits"), stream=stream, pcm16=op.p["pcm16"])


class DecDistortion(DecCrops):
    """decode_crops_distortion_dev: the rows' coded spectra summed against seeded reference planes (distortion_testlib's referee)."""
    name, exports, n_seg = "decode_crops_distortion", ("ulcx_decode_crops_distortion_dev",), 4

    def apply(self, m, op):
        import distortion_testlib as D
        c, inp = self.corpus_in(m)
        files, first, count = (np.array(x, np.int32) for x in zip(*op.p["rows"]))
        ref = D.ref_planes(len(files), m.ch, op.p["N"], m.bs, seed=7 + op.hint["j"])
        dist, wc, bits = D.expected_rows(c, files, first, op.p["N"], self.n_seg, ref=ref, count=count, lr=op.p["pcm16"])
        inp.update(file=files, first=first, cnt=count, ref=ref)
        return inp, dict(dist=dist, wc=wc, bits=bits)

    def call(self, obj, op, P, stream, aux):
        c, n = corpus(obj.BS, obj.C), len(op.p["rows"])
        obj.decode_crops_distortion_dev(*self.corpus_args(c, P), n, P("file"), P("first"), P("cnt"), op.p["N"], P("ref"), n, op.p["N"], 0, 0, self.n_seg,
                                        1 if op.p["pcm16"] else 0, P("dist"), P("wc"), P("bits"), stream=stream)


class DecSplice(_Stateless):
    """corpus_splice_dev: new files from block ranges of the corpus's clean files - two files joined, a tail, an empty file."""
    name, exports, istride = "corpus_splice", ("ulcx_corpus_splice_dev",), 8

    def lazy(self, m, op):
        return []

    def plan(self, m, op, rng):
        c = corpus(m.bs, m.ch)
        clean, j = c.F - 1, op.hint["j"]
        f1 = (clean - 1) if clean > 1 else 0
        op.p.update(files=[[(0, 2 + j % 5, 3), (f1, 1 + j % 3, 2)], [(0, c.K[0] - 2, 2)], [], [(f1, j % 7, 1), (0, 4, 0), (0, 9, 2)]])

    def apply(self, m, op):
        import splice_testlib as S
        c = corpus(m.bs, m.ch)
        stride = 6 * (2 * m.ch * m.bs + 16)
        exp, starts = S.expected(c, op.p["files"], stride, self.istride)
        offs, seg = S.seg_arrays(op.p["files"])
        n = len(exp)
        payload, mask = np.zeros((n, stride), np.uint8), np.zeros((n, stride), bool)
        for o, e in enumerate(exp):
            payload[o, :e.nbytes] = e.payload
            mask[o, :e.nbytes] = True
        inp = dict(payload=c.host, nbytes=c.nbytes, index=c.index, count=c.count, seg_offs=offs, seg=seg)
        return inp, dict(out_payload=(payload, mask), out_bytes=np.array([e.nbytes for e in exp], np.int32), out_max=np.array([e.max_block for e in exp], np.int32),
                         out_index=np.stack([e.index for e in exp]).view(np.int32).reshape(n, -1), out_count=np.array([e.n for e in exp], np.int32),
                         seg_start=starts)

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.corpus_splice_dev(*self.corpus_args(c, P), len(op.p["files"]), P("seg_offs"), P("seg"), aux["seg"].shape[0], P("out_payload"),
                              6 * (2 * obj.C * obj.BS + 16), P("out_bytes"), P("out_max"), P("out_index"), self.istride, P("out_count"), P("seg_start"),
                              stream=stream)


class DecSynth(_Stateless):
    """synth_spectra_dev: PCM from the planes the oracle's decoder holds for rows of the corpus, with the block in front (warm)."""
    name, exports = "synth_spectra", ("ulcx_synth_spectra_dev", "ulcx_synth_spectra_dev_pcm16")

    def plan(self, m, op, rng):
        c = corpus(m.bs, m.ch)
        n, n_out = min(op.hint["n8"], m.B), min(op.hint["N3"], m.maxK - 2)
        rows = []
        for _ in range(n):
            f = int(rng.integers(0, c.F - 1))
            rows.append((f, int(rng.integers(1, c.K[f] - n_out))))
        op.p.update(rows=rows, N=n_out, pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        import synth_spectra_testlib as S
        c = corpus(m.bs, m.ch)
        r = [S.row(c.files[f], first, op.p["N"], 1) for f, first in op.p["rows"]]
        pcm = np.stack([x[2] for x in r])
        return (dict(coef=np.stack([x[0] for x in r]), wc=np.stack([x[1] for x in r])),
                dict(pcm=to_pcm16(pcm) if op.p["pcm16"] else pcm, live=np.stack([x[3] for x in r])))

    def call(self, obj, op, P, stream, aux):
        obj.synth_spectra_dev(len(op.p["rows"]), op.p["N"] + 1, 2, P("coef"), P("wc"), P("pcm"), P("live"), stream=stream, pcm16=op.p["pcm16"])


class DecIndexRows(_Stateless):
    """index_packed_rows_dev over the corpus's clean files: the oracle's walk (File.row), cut at maxBlocks."""
    name, exports = "index_packed_rows", ("ulcx_index_packed_rows_dev",)

    def lazy(self, m, op):
        return []

    def plan(self, m, op, rng):
        c = corpus(m.bs, m.ch)
        op.p.update(max_blocks=int(max(c.K) if op.hint["j"] & 1 else min(c.K) - 3))

    def apply(self, m, op):
        c, mb = corpus(m.bs, m.ch), op.p["max_blocks"]
        F = c.F - 1
        index = np.stack([c.files[f].row(mb + 1, min(c.K[f], mb)) for f in range(F)])
        return (dict(payload=c.host[:F], nbytes=c.nbytes[:F]),
                dict(index=index.view(np.int32).reshape(F, -1), count=np.array([min(c.K[f], mb) for f in range(F)], np.int32)))

    def call(self, obj, op, P, stream, aux):
        c = corpus(obj.BS, obj.C)
        obj.index_packed_rows_dev(c.F - 1, P("payload"), c.host.shape[1], P("nbytes"), op.p["max_blocks"], P("index"), P("count"), stream=stream)


class DecIndexSlots(_Stateless):
    """index_begin_dev + index_slots_dev: the index of slot-form rows (what an encode call wrote), appended in two calls."""
    name, exports = "index_slots", ("ulcx_index_begin_dev", "ulcx_index_slots_dev")

    def lazy(self, m, op):
        return []

    def plan(self, m, op, rng):
        op.p.update(K=min(op.hint["N3"], m.maxK), n=min(op.hint["n8"], 5))

    def apply(self, m, op):
        K, n = op.p["K"], op.p["n"]
        files = [dec_file(m.bs, m.ch, i % m.B) for i in range(n)]
        blocks = np.stack([f.blocks[:2 * K] for f in files]).reshape(n, 2, K, -1)
        bits = np.stack([f.bits[:2 * K] for f in files]).reshape(n, 2, K)
        index = np.stack([f.row(2 * K + 2, 2 * K) for f in files])
        return (dict(b0=np.ascontiguousarray(blocks[:, 0]), b1=np.ascontiguousarray(blocks[:, 1]), bits0=np.ascontiguousarray(bits[:, 0]),
                     bits1=np.ascontiguousarray(bits[:, 1])),
                dict(index=index.view(np.int32).reshape(n, -1), count=np.full(n, 2 * K, np.int32)))

    def call(self, obj, op, P, stream, aux):
        K, n, slot = op.p["K"], op.p["n"], 2 * obj.C * obj.BS + 16
        obj.index_begin_dev(n, P("index"), 2 * K + 2, P("count"), stream=stream)
        obj.index_slots_dev(n, P("b0"), slot, P("bits0"), K, P("index"), 2 * K + 2, P("count"), stream=stream)
        obj.index_slots_dev(n, P("b1"), slot, P("bits1"), K, P("index"), 2 * K + 2, P("count"), stream=stream)


# ---- encoder, streaming ---------------------------------------------------------------------------------------------
def _coded(rows, lead=()):
    """rows of EncModel.feed -> the expected out / bits / wc / cplx of a block-form call; of `out` only bytes [0, bits / 8) are defined"""
    out, bits = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    mask = np.arange(out.shape[-1])[None, None, :] < (bits[:, :, None] // 8)
    return dict(out=(out, mask), bits=bits, wc=np.stack([r[2] for r in rows]).astype(np.int32), cplx=np.stack([r[3] for r in rows]).astype(np.float32))


class EncPlain(Family):
    kind, name, exports = "enc", "encode", ("ulcx_encode_dev",)
    setting, pcm16 = VBR50, False

    def plan(self, m, op, rng):
        op.p.update(K=_K_all(m, op.hint["K"]))

    def settings(self, m, slots):
        return [self.setting for _ in slots]

    def apply(self, m, op):
        K, slots = op.p["K"], [int(s) for s in op.p.get("slots", range(m.B))]
        x = np.stack([m.pcm_in(s, K) for s in slots])
        st = self.settings(m, slots)
        exp = _coded([m.feed(s, K, t) for s, t in zip(slots, st)])
        inp = dict(pcm=np.rint(x * 32768.0).astype(np.int16) if self.pcm16 else x, rate=np.array(st, np.float32))
        if "slots" in op.p:
            inp["slots"] = op.p["slots"]
        return inp, exp

    def call(self, obj, op, P, stream, aux):
        mode, p0, p1 = mode_of(self.setting)
        fn = obj.encode_dev_pcm16 if self.pcm16 else obj.encode_dev
        fn(P("pcm"), op.p["K"], P("out"), P("bits"), P("wc"), P("cplx"), mode=mode, p0=p0, p1=p1, stream=stream)


class EncPlain16(EncPlain):
    name, exports, setting, pcm16 = "encode_pcm16", ("ulcx_encode_dev_pcm16",), CBR64, True


class EncRates(EncPlain):
    name, exports = "encode_rates", ("ulcx_encode_dev_rates", "ulcx_encode_dev_pcm16_rates")

    def plan(self, m, op, rng):
        super().plan(m, op, rng)
        op.p.update(pcm16=bool(op.hint["j"] & 1))

    def settings(self, m, slots):
        return [m.setting(s) for s in slots]

    def apply(self, m, op):
        self.pcm16 = op.p["pcm16"]
        return super().apply(m, op)

    def call(self, obj, op, P, stream, aux):
        obj.encode_dev_rates(P("rate"), P("pcm"), op.p["K"], P("out"), P("bits"), P("wc"), P("cplx"), stream=stream, pcm16=op.p["pcm16"])


class EncSubset(EncPlain):
    """encode_subset_dev: float and int16 input, the scalar setting and a table per row, in turn."""
    name, exports = "encode_subset", ("ulcx_encode_dev_subset", "ulcx_encode_dev_pcm16_subset")

    def lazy(self, m, op):
        return [("enc_shadow", 1)]

    def plan(self, m, op, rng):
        slots = _slot_list(m, rng, op.hint["n"], 1)
        op.p.update(slots=slots, K=max(1, min(op.hint["K"], min(m.room(int(s)) for s in slots))), pcm16=bool(op.hint["j"] & 1), table=bool(op.hint["j"] & 2))

    def settings(self, m, slots):
        return [m.setting(s) if self._table else CBR64 for s in slots]

    def apply(self, m, op):
        self.pcm16, self._table = op.p["pcm16"], op.p["table"]
        return super().apply(m, op)

    def call(self, obj, op, P, stream, aux):
        mode, p0, p1 = mode_of(CBR64)
        obj.encode_subset_dev(P("slots"), len(op.p["slots"]), P("pcm"), op.p["K"], P("out"), P("bits"), P("wc"), P("cplx"), mode=mode, p0=p0, p1=p1,
                              d_rates=P("rate") if op.p["table"] else 0, stream=stream, pcm16=op.p["pcm16"])


class EncAnalyse(EncPlain):
    name, exports = "analyse", ("ulcx_analyse_dev", "ulcx_analyse_dev_pcm16")

    def plan(self, m, op, rng):
        super().plan(m, op, rng)
        op.p.update(pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        self.pcm16 = op.p["pcm16"]
        inp, exp = super().apply(m, op)
        return inp, dict(wc=exp["wc"], cplx=exp["cplx"])

    def call(self, obj, op, P, stream, aux):
        obj.analyse_dev(P("pcm"), op.p["K"], P("wc"), P("cplx"), stream=stream, pcm16=op.p["pcm16"])


class EncAnalyseSubset(EncSubset):
    name, exports = "analyse_subset", ("ulcx_analyse_dev_subset",)

    def apply(self, m, op):
        op.p.update(pcm16=False, table=False)
        inp, exp = super().apply(m, op)
        return inp, dict(wc=exp["wc"], cplx=exp["cplx"])

    def call(self, obj, op, P, stream, aux):
        obj.analyse_subset_dev(P("slots"), len(op.p["slots"]), P("pcm"), op.p["K"], P("wc"), P("cplx"), stream=stream)


def _ladder_model(m, K, rungs):
    """a ladder call's outputs: every rung the oracle's run under that rung's setting of the same blocks; the state advances once"""
    a = list(m.pos)
    per = []
    for g in rungs:
        m.pos = list(a)
        per.append(_coded([m.feed(s, K, m.setting(s) if g == "table" else g) for s in range(m.B)]))
    out = np.stack([p["out"][0] for p in per]), np.stack([p["out"][1] for p in per])
    return dict(out=out, bits=np.stack([p["bits"] for p in per]), wc=per[0]["wc"], cplx=per[0]["cplx"])


def _lib_rungs(rungs, table):
    return [table if g == "table" else mode_of(g) for g in rungs]


class EncLadder(Family):
    """encode_dev_ladder: two rungs, later four; a table rung among them."""
    kind, name, exports = "enc", "encode_ladder", ("ulcx_encode_dev_ladder", "ulcx_encode_dev_pcm16_ladder")

    def plan(self, m, op, rng):
        op.p.update(K=_K_all(m, op.hint["K"]), rungs=LADDER2 if op.hint["j"] < 2 else LADDER4, pcm16=bool(op.hint["j"] & 1))

    def apply(self, m, op):
        K = op.p["K"]
        x = np.stack([m.pcm_in(s, K) for s in range(m.B)])
        rate = np.array([m.setting(s) for s in range(m.B)], np.float32)
        return dict(pcm=np.rint(x * 32768.0).astype(np.int16) if op.p["pcm16"] else x, rate=rate), _ladder_model(m, K, op.p["rungs"])

    def call(self, obj, op, P, stream, aux):
        obj.encode_dev_ladder(_lib_rungs(op.p["rungs"], P("rate")), P("pcm"), op.p["K"], P("out"), P("bits"), P("wc"), P("cplx"), stream=stream,
                              pcm16=op.p["pcm16"])


class EncHostLadder(EncLadder):
    """ulcx_encode_host_ladder: the object's rung staging (ladOut / ladRungs) grows when a call brings more rungs than any before."""
    name, host, exports = "encode_host_ladder", True, ("ulcx_encode_host_ladder",)

    def lazy(self, m, op):
        return [("enc_host_staging", 1), ("lad_staging", len(op.p["rungs"]))]

    def apply(self, m, op):
        op.p["pcm16"] = False
        m.lad_rungs = max(m.lad_rungs, len(op.p["rungs"]))
        return super().apply(m, op)

    def call(self, obj, op, inp):
        K = op.p["K"]
        out, bits, wc, cplx = obj.encode_ladder(inp["pcm"].reshape(obj.B, K * obj.BS, obj.C), _lib_rungs(op.p["rungs"], inp["rate"]))
        return dict(out=out, bits=bits, wc=wc, cplx=cplx)


class EncHost(EncPlain):
    name, host, exports = "encode_host", True, ("ulcx_encode_host",)

    def lazy(self, m, op):
        return [("enc_host_staging", 1)]

    def call(self, obj, op, inp):
        mode, p0, p1 = mode_of(self.setting)
        out, bits, wc, cplx = obj.encode(inp["pcm"].reshape(obj.B, op.p["K"] * obj.BS, obj.C), mode=mode, p0=p0, p1=p1)
        return dict(out=out, bits=bits, wc=wc, cplx=cplx)


# ---- encoder, stateless: clips (no slot of the encoder is read or changed) ---------------------------------------------------
def clip_case(bs):
    """nSamples and the seven lengths of the axis's clips: ten blocks at the most, two chunks of maxBlocksPerCall = 8"""
    import clips_testlib as ct
    T = 7 * bs + 3
    return ct.Case(T, (0, 1, bs - 1, bs, bs + 1, 3 * bs + 7, T))


CLIP_ROWS = (6, 1, 4, 0, 5)                                # pairs of the call's rows: the longest first, an empty clip among them
CLIP_RUNGS2 = (("scalar", VBR50), ("table",))
CLIP_RUNGS4 = (("scalar", VBR50), ("table",), ("scalar", CBR64), ("auto", 96.0))     # one ULCX_RUNG_AUTO rung


def _clip_files(refs, pstride, istride):
    """[file] ClipRefs -> the expected corpus of a clips call: payload (bytes [0, payload_bytes) defined), sizes, index, counts"""
    F = len(refs)
    payload, mask = np.zeros((F, pstride), np.uint8), np.zeros((F, pstride), bool)
    nbytes, maxb, count = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32)
    index = []
    for f, r in enumerate(refs):
        m_ = r.kept(pstride, istride)
        assert m_ == r.nb
        nbytes[f], count[f], maxb[f] = r.payload.size, r.nb, int(r.sizes.max()) if r.nb else 0
        payload[f, :r.payload.size] = r.payload
        mask[f, :r.payload.size] = True
        index.append(r.index_row(istride, m_))
    return dict(payload=(payload, mask), nbytes=nbytes, maxb=maxb, index=np.stack(index).view(np.int32).reshape(F, -1), count=count)


class EncClips(Family):
    kind, name, streaming, exports = "enc", "encode_clips", False, ("ulcx_encode_clips_dev", "ulcx_encode_clips_dev_pcm16")

    def lazy(self, m, op):
        return [("enc_shadow", 1), ("clips_staging", 1), ("clip_scratch", 1)]

    def plan(self, m, op, rng):
        op.p.update(rows=CLIP_ROWS[:min(len(CLIP_ROWS), m.B)], pcm16=bool(op.hint["j"] & 1), table=bool(op.hint["j"] & 2))

    def geometry(self, m):
        import clips_testlib as ct
        case = clip_case(m.bs)
        nb = ct.clip_blocks(m.bs, case.T)
        return ct, case, (2 * m.ch * m.bs + 16) * nb, nb + 1

    def clip_in(self, m, op):
        ct, case, pstride, istride = self.geometry(m)
        rows = list(op.p["rows"])
        w = ct.wave(m.bs, m.ch, case.T)[rows]
        return dict(pcm=to_pcm16(w) if op.p["pcm16"] else w, len=np.array(case.lengths, np.int32)[rows], rate=np.array(ct.TABLE, np.float32)[rows])

    def apply(self, m, op):
        ct, case, pstride, istride = self.geometry(m)
        m.clip_rungs = max(m.clip_rungs, 1)
        refs = [ct.row_ref(m.bs, m.ch, i, op.p["table"], case) for i in op.p["rows"]]
        return self.clip_in(m, op), _clip_files(refs, pstride, istride)

    def call(self, obj, op, P, stream, aux):
        ct, case, pstride, istride = self.geometry(aux["model"])
        obj.encode_clips_dev(aux["dec"], len(op.p["rows"]), P("pcm"), P("len"), case.T, P("payload"), pstride, P("nbytes"), P("index"), istride,
                             P("count"), d_max_block=P("maxb"), mode=0, p0=50.0, d_rates=P("rate") if op.p["table"] else 0, stream=stream,
                             pcm16=op.p["pcm16"])


class EncClipsLadder(EncClips):
    """encode_clips_ladder_dev: two rungs, later four with one ULCX_RUNG_AUTO rung - clips_staging regrows for the wider call."""
    name, exports = "encode_clips_ladder", ("ulcx_encode_clips_ladder_dev", "ulcx_encode_clips_ladder_dev_pcm16")

    def lazy(self, m, op):
        return [("enc_shadow", 1), ("clips_staging", len(op.p["rungs"])), ("clip_scratch", 1)] + ([("clip_auto", 1)] if len(op.p["rungs"]) > 2 else [])

    def plan(self, m, op, rng):
        op.p.update(rows=CLIP_ROWS[:min(len(CLIP_ROWS), m.B)], pcm16=bool(op.hint["j"] & 1), rungs=CLIP_RUNGS2 if op.hint["j"] < 2 else CLIP_RUNGS4)

    def apply(self, m, op):
        import clips_ladder_testlib as cl
        ct, case, pstride, istride = self.geometry(m)
        m.clip_rungs = max(m.clip_rungs, len(op.p["rungs"]))
        refs = [cl.file_ref(m.bs, m.ch, i, g, case) for g in op.p["rungs"] for i in op.p["rows"]]
        exp = _clip_files(refs, pstride, istride)
        if any(cl.is_auto(g) for g in op.p["rungs"]):
            exp["avg"] = np.array([cl.avg(m.bs, m.ch, i, case) for i in op.p["rows"]], np.float32)
        return self.clip_in(m, op), exp

    def call(self, obj, op, P, stream, aux):
        import clips_ladder_testlib as cl
        ct, case, pstride, istride = self.geometry(aux["model"])
        auto = any(cl.is_auto(g) for g in op.p["rungs"])
        obj.encode_clips_ladder_dev(aux["dec"], len(op.p["rows"]), cl.lib_rungs(op.p["rungs"], P("rate")), P("pcm"), P("len"), case.T, P("payload"), pstride,
                                    P("nbytes"), P("index"), istride, P("count"), d_max_block=P("maxb"), d_avg=P("avg") if auto else 0, stream=stream,
                                    pcm16=op.p["pcm16"])


class EncAnalyseClips(EncClips):
    """analyse_clips_dev: the encoder's own MDCT coefficients, window codes and complexities of the clips' leading blocks."""
    name, exports = "analyse_clips", ("ulcx_analyse_clips_dev", "ulcx_analyse_clips_dev_pcm16")
    depth = 5

    def lazy(self, m, op):
        return [("enc_shadow", 1), ("clip_scratch", 1)]

    def planes(self, m, op):
        import clip_spectra_testlib as cs
        case = clip_case(m.bs)
        coef, wc, cplx = cs.expected([cs.row_spec(m.bs, m.ch, i, case) for i in op.p["rows"]], self.depth, lr=op.p["table"])
        return dict(coef=coef, wc=wc, cplx=cplx)

    def apply(self, m, op):
        return self.clip_in(m, op), self.planes(m, op)

    def call(self, obj, op, P, stream, aux):
        obj.analyse_clips_dev(len(op.p["rows"]), P("pcm"), P("len"), clip_case(obj.BS).T, self.depth, P("coef"), P("wc"), P("cplx"),
                              flags=1 if op.p["table"] else 0, stream=stream, pcm16=op.p["pcm16"])


class EncClipsSpectra(EncAnalyseClips):
    """encode_clips_spectra_dev: the clips call's corpus and the tap's planes of the same blocks (scalar VBR 50)."""
    name, exports = "encode_clips_spectra", ("ulcx_encode_clips_spectra_dev", "ulcx_encode_clips_spectra_dev_pcm16")

    def lazy(self, m, op):
        return [("enc_shadow", 1), ("clips_staging", 1), ("clip_scratch", 1), ("clip_spec", 1)]

    def apply(self, m, op):
        ct, case, pstride, istride = self.geometry(m)
        m.clip_rungs = max(m.clip_rungs, 1)
        exp = _clip_files([ct.row_ref(m.bs, m.ch, i, False, case) for i in op.p["rows"]], pstride, istride)
        exp.update(self.planes(m, op))
        return self.clip_in(m, op), exp

    def call(self, obj, op, P, stream, aux):
        ct, case, pstride, istride = self.geometry(aux["model"])
        obj.encode_clips_spectra_dev(aux["dec"], len(op.p["rows"]), P("pcm"), P("len"), case.T, P("payload"), pstride, P("nbytes"), P("index"), istride,
                                     P("count"), self.depth, P("coef"), P("wc"), P("cplx"), flags=1 if op.p["table"] else 0, d_max_block=P("maxb"),
                                     mode=0, p0=50.0, stream=stream, pcm16=op.p["pcm16"])


def families(kind, geom):
    """The family table of an object kind at a geometry, in a fixed order: {name: Family}.  (A low-rate ratio whose reduced
    BlockSize is no legal one at the geometry has no family there.)"""
    bs = geom[0]
    if kind == "dec":
        fams = [DecPlain(), DecPlain16(), DecSubset(), DecSubset16(), DecPacked(), DecRange(), DecResident(), DecHost(),
                _slot_family(Reset, "dec", "decoder")(), _slot_family(Save, "dec", "decoder")(), _slot_family(Load, "dec", "decoder")(),
                DecCrops(), DecCropsRagged(), DecSamples()] + [DecLowrate(l) for l in (1, 2, 3) if (bs >> l) >= 256] + \
               [DecSpectra(), DecDistortion(), DecSynth(), DecSplice(), DecIndexRows(), DecIndexSlots()]
    else:
        fams = [EncPlain(), EncPlain16(), EncRates(), EncSubset(), EncAnalyse(), EncAnalyseSubset(), EncLadder(), EncHost(), EncHostLadder(),
                _slot_family(Reset, "enc", "encoder")(), _slot_family(Save, "enc", "encoder")(), _slot_family(Load, "enc", "encoder")(),
                EncClips(), EncClipsLadder(), EncClipsSpectra(), EncAnalyseClips()]
    return {f.name: f for f in fams}


FAMILIES = {kind: families(kind, (2048, 2, 0, 0)) for kind in ("dec", "enc")}          # the full table (the binding test's)

# The _dev entries of the binding's two signature tables that take an object and belong to no family of the sequences, the
# single-block calls and the debug hooks, each with its reason.  tests/test_call_axis_capi.py holds the tables against this.
_RAGGED = "the ragged layout of a sequenced family: one corpus view serves both layouts, and decode_crops_ragged puts that view into the sequences"
NOT_SEQUENCED = {
    "ulcx_encode_block1": "needs an object of one stream and one block per call (tests/test_gpu_dropin.py)",
    "ulcx_decode_block1": "needs an object of one stream and one block per call (tests/test_gpu_dropin.py)",
    "ulcx_decode_block1_rng": "needs an object of one stream and one block per call (tests/test_gpu_dropin.py)",
    "ulcx_encoder_debug_fetch": "debug hook: reads the taps of the last call", "ulcx_encoder_debug_writer_flags": "debug hook: reads the last call's tiers",
    "ulcx_encoder_debug_front_plan": "debug hook: host arithmetic", "ulcx_encoder_debug_writer_plan": "debug hook: host arithmetic",
    "ulcx_encoder_debug_plan": "debug hook: host arithmetic", "ulcx_encoder_debug_force_exact": "debug hook: changes the path of later calls, not their results",
    "ulcx_index_packed_dev": "index_packed_rows is the same body for any number of rows",
    "ulcx_index_packed_ragged_dev": _RAGGED,
    "ulcx_decode_crops_samples_ragged_dev": _RAGGED, "ulcx_decode_crops_samples_ragged_dev_pcm16": _RAGGED,
    "ulcx_decode_crops_lowrate_ragged_dev": _RAGGED, "ulcx_decode_crops_lowrate_ragged_dev_pcm16": _RAGGED,
    "ulcx_decode_crops_spectra_ragged_dev": _RAGGED,
    "ulcx_decode_crops_distortion_ragged_dev": _RAGGED, "ulcx_corpus_splice_ragged_dev": _RAGGED,
}


# ---------------------------------------------------------------------------------------------------------------------
# sequence(): every ordered pair of families as consecutive calls
# ---------------------------------------------------------------------------------------------------------------------
def euler_walk(names, start, seed):
    """An Eulerian circuit of the complete digraph with self-loops over `names`, from `start`: len(names) ** 2 + 1 vertices, every
    ordered pair (A, B) once as consecutive entries.  Hierholzer's algorithm with the edges of every vertex in a seeded order."""
    rng = np.random.default_rng(seed)
    left = {a: [names[i] for i in rng.permutation(len(names))] for a in names}
    stack, walk = [start], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == len(names) ** 2 + 1 and {(a, b) for a, b in zip(walk, walk[1:])} == {(a, b) for a in names for b in names}
    return walk


ENC_LONG = ("encode", "encode_subset", "analyse_subset", "encode_ladder", "encode_rates")      # the encoder families whose fourth call has maxK blocks
AFTER_CUT = ("save_streams", "load_streams", "reset_streams", "decode_subset", "decode_packed", "decode_range", "decode_crops")


class Prepared:
    """A call with its inputs and what it must write."""

    def __init__(self, op, fam, inputs, expected):
        self.op, self.fam, self.inputs, self.expected = op, fam, inputs, expected


class Sequence:
    def __init__(self, kind, name, geom, start, calls, model, lazy_events, prologue):
        self.kind, self.name, self.geom, self.start, self.calls, self.model, self.lazy_events = kind, name, geom, start, calls, model, lazy_events
        self.prologue = prologue                            # calls in front of the walk (start b: the lazy pieces' builders)


def _family_order(kind, fams, start, seed):
    """-> (the families of the sequence's calls in order, the length of the prologue).  Start a: the walk, from a streaming call.
    Start b: in front of the walk a prologue that builds and grows every lazy piece - every stateless family once, the ones
    whose third call grows a staging three times, then the streaming families that build a piece of their own."""
    names = list(fams)
    walk = euler_walk(names, next(n for n in names if fams[n].streaming), seed)
    if start == "a":
        return walk, 0
    pro = []
    for n in names:
        if not fams[n].streaming:
            pro += [n] * (3 if n == "encode_clips_ladder" else 1)
    for n in ("decode_subset", "encode_subset", "decode_host", "encode_host", "encode_host_ladder", "resident"):
        if n in fams:
            pro += [n] * (3 if n in ("decode_host", "encode_host_ladder") else 1)
    return pro + walk, len(pro)


@functools.lru_cache(maxsize=None)
def sequence(kind, name, start="a", seed=1, device_only=False):
    """The prepared calls of object kind `kind` at geometry GEOMS[kind][name]: the family order (an Eulerian walk; start b: the
    lazy pieces' builders in front of it), parameters planned from the model's state - K from {1, 3, maxK}, slot lists of 1, 5 or
    65 slots, crop calls of at most 8 rows of at most 3 blocks - and every call's inputs and expected outputs.  device_only: the
    same order without the host forms (their calls change state, so the chain is planned on its own)."""
    geom = GEOMS[kind][name]
    fams = families(kind, geom)
    model = (DecModel if kind == "dec" else EncModel)(geom)
    rng = np.random.default_rng([seed, geom[0], geom[2], kind == "dec"])
    order, prologue = _family_order(kind, fams, start, seed)
    prologue = len([n for n in order[:prologue] if not (device_only and fams[n].host)])
    order = [n for n in order if not (device_only and fams[n].host)]
    maxK = geom[3]
    seen, calls, levels, events = {}, [], {}, []
    cuts_here = bool(predicted_cut(geom[0], geom[1], 1, maxK))
    need_cut = {n for n in fams if fams[n].cuts} if cuts_here else set()
    need_after = set(AFTER_CUT) if need_cut else set()
    for i, fname in enumerate(order):
        fam = fams[fname]
        j = seen.get(fname, 0)
        seen[fname] = j + 1
        nxt = order[i + 1] if i + 1 < len(order) else None
        K = (1, 3, 1, 1)[j % 4] if kind == "dec" else (1, 1, 3, 1, 1, 1)[j % 6]
        if kind == "dec" and fam.cuts and (fname in need_cut or nxt in need_after):
            K = maxK
        elif j == 3 and (fname in ENC_LONG or (kind == "dec" and fam.cuts and not cuts_here)):
            K = maxK                                        # (a geometry that is never cut: the long call all the same)
        hint = dict(j=j, K=K, n=(1, 5, 65)[j % 3], n8=(8, 3, 5)[j % 3], N3=(3, 1, 2)[j % 3], behind_cut=bool(calls and calls[-1].op.p.get("cut")))
        op = Op(i, fname, order[i - 1] if i else None, j == 0, hint)
        fam.plan(model, op, rng)
        if kind == "dec" and fam.cuts:
            n_rows = len(op.p["slots"]) if "slots" in op.p else geom[2]
            Kc = op.p["K"]
            op.p["cut"] = predicted_cut(geom[0], geom[1], n_rows, Kc)
            if op.p["cut"]:
                need_cut.discard(fname)
                need_after.discard(nxt)
        for piece, level in fam.lazy(model, op):
            if levels.get(piece, 0) < level:
                events.append((piece, "build" if piece not in levels else "grow", i))
                levels[piece] = level
        inputs, expected = fam.apply(model, op)
        calls.append(Prepared(op, fam, inputs, expected))
    return Sequence(kind, name, geom, start, calls, model, events, prologue)


# ---------------------------------------------------------------------------------------------------------------------
# run(): a sequence against a backend, every output of every call against the model
# ---------------------------------------------------------------------------------------------------------------------
class AxisFailure(AssertionError):
    pass


def compare(call, got):
    """-> the first difference between a call's outputs and what the model says, or None"""
    for name, want in call.expected.items():
        if name not in got:
            return f"output {name} missing"
        want, mask = want if isinstance(want, tuple) else (want, None)
        g = np.asarray(got[name])
        if g.size != want.size:
            return f"{name}: {g.shape} in place of {want.shape}"
        g = g.reshape(want.shape)
        a, b = np.ascontiguousarray(g).view(np.uint8).reshape(want.shape + (-1,)), np.ascontiguousarray(want).view(np.uint8).reshape(want.shape + (-1,))
        bad = (a != b).any(axis=-1)
        if mask is not None:
            bad &= mask
        if bad.any():
            where = tuple(int(x[0]) for x in np.nonzero(bad))
            return f"{name}: {int(bad.sum())} of {bad.size} elements differ from the oracle's, first at {where}: {g[where]!r} in place of {want[where]!r}"
    return None


def fail(call, what):
    op = call.op
    raise AxisFailure(f"op {op.i}, {op.prev or 'create'} -> {op.family} ({'the first' if op.first else 'not the first'} {op.family} call of the object; "
                      f"{ {k: (v.tolist() if isinstance(v, np.ndarray) and v.size <= 8 else v) for k, v in op.p.items() if k != 'rows'} }): {what}")


def run(calls, backend, identity=True, after=None):
    """Every call through backend.run(call) -> outputs, compared at once.  identity: around every stateless call backend.state() -
    save_streams of all slots - must not change.  after(call): the caller's hook behind every call."""
    for call in calls:
        before = backend.state() if identity and not call.fam.streaming else None
        got = backend.run(call)
        what = compare(call, got)
        if what:
            fail(call, what)
        if before is not None and not _same_state(before, backend.state()):
            fail(call, "save_streams of all slots changed around a call that leaves stream state alone")
        if after:
            after(call)


def _same_state(a, b):
    return a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b


class StandIn:
    """An object made of the model itself: it answers every call from its own copy of the model's state, so a sequence run against
    it passes - unless a fault is planted, which the run must then report:
      "stale_set"     after a cut call, save_streams still reads the state set of before the call
      "shadow_back"   a stateless family writes one slot's shadow state (what the last subset call gathered) back
      "lost_chunk"    growing the rung staging loses what was staged before: the first wider ladder call gives its first rungs empty"""

    def __init__(self, seq, fault=None):
        self.model = type(seq.model)(seq.geom)
        self.fault, self.stale, self.shadow, self.rungs = fault, None, None, 0

    def state(self):
        return copy.deepcopy(self.model.state())

    def run(self, call):
        m, op, fam = self.model, call.op, call.fam
        pre = [m.snapshot(s) for s in range(m.B)]
        if self.fault == "shadow_back" and not fam.streaming and self.shadow is not None:
            m.restore(*self.shadow)
        if "subset" in op.family:
            self.shadow = (int(op.p["slots"][0]), pre[int(op.p["slots"][0])])
        _, out = fam.apply(m, copy.copy(op))
        if self.fault == "stale_set" and op.family == "save_streams" and self.stale is not None:
            m.records[op.p["rec"]] = [self.stale[int(s)] for s in op.p["slots"]]
        self.stale = pre if op.p.get("cut") else None
        out = {k: (v[0] if isinstance(v, tuple) else v) for k, v in out.items()}
        if "rungs" in op.p:
            if self.fault == "lost_chunk" and 0 < self.rungs < len(op.p["rungs"]):
                lost = "payload" if "payload" in out else "out"
                out[lost] = out[lost].copy()
                n = out[lost].shape[0] * self.rungs // len(op.p["rungs"])
                out[lost].reshape(out[lost].shape[0], -1)[:n] = 0
            self.rungs = max(self.rungs, len(op.p["rungs"]))
        return out


class GpuBackend:
    """The library on the GPU.  One object per backend; run(call) uploads the inputs, poisons the outputs, makes the call and
    synchronises.  prepare() / enqueue() / fetch() split that for a chain of calls that nothing waits for: every buffer of every call
    is made beforehand and stays alive until fetch()."""

    def __init__(self, seq, dec=None):
        import torch
        from gpu_testlib import amd
        self.t, self.amd, self.seq = torch, amd(), seq
        bs, ch, B, maxK = seq.geom
        self.obj = self.amd.BatchDecoder(B, ch, bs, maxK) if seq.kind == "dec" else self.amd.BatchEncoder(B, ch, bs, RATE, maxK)
        self.dec, self.owns_dec = dec, False                # an encoder's clips calls take a decoder of its geometry: the caller's, or one of its own
        if seq.kind == "enc" and dec is None:
            g = DEC_GEOMS["2048x2x6" if bs == 2048 else "512x1x9"]
            self.dec, self.owns_dec = self.amd.BatchDecoder(g[2], g[1], g[0], g[3]), True
        self.records, self.cuts = {}, []
        self.dev = torch.device("cuda", 0)

    def close(self):
        self.obj.close()
        if self.owns_dec:
            self.dec.close()

    def state(self):
        self.t.cuda.synchronize()
        return self.obj.save_streams(list(range(self.obj.B)))

    def _up(self, a):
        a = np.ascontiguousarray(a)
        return self.t.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.dev)

    def _buffers(self, call):
        """device copies of the inputs, poisoned outputs, the record buffers the call names -> ({name: tensor}, {name: (shape, dtype)})"""
        t, bufs = self.t, {k: self._up(v) for k, v in call.inputs.items()}
        outs = call.fam.outs(call.expected)
        for k, (shape, dtype) in outs.items():
            bufs[k] = t.full((max(1, int(np.prod(shape)) * np.dtype(dtype).itemsize),), POISON, dtype=t.uint8, device=self.dev)
        rec = call.op.p.get("rec", "absent")
        if call.op.family == "save_streams":
            self.records[rec] = t.full((len(call.op.p["slots"]) * self.obj.state_bytes,), POISON, dtype=t.uint8, device=self.dev)
        if call.op.family == "load_streams" and rec is None and None not in self.records:
            fresh = type(self.obj)(*((1, self.obj.C, self.obj.BS, 1) if self.seq.kind == "dec" else (1, self.obj.C, self.obj.BS, RATE, 1)))
            self.records[None] = self._up(np.repeat(fresh.save_streams([0]), self.obj.B, axis=0))
            fresh.close()
        return bufs, outs

    def _launch(self, call, bufs, stream):
        def P(name):
            return self.records[None if name == "rec:None" else int(name[4:])].data_ptr() if name.startswith("rec:") else bufs[name].data_ptr()
        call.fam.call(self.obj, call.op, P, stream, dict(call.inputs, dec=self.dec, model=self.seq.model))

    def _down(self, bufs, outs):
        return {k: bufs[k].cpu().numpy()[:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape) for k, (shape, dtype) in outs.items()}

    def run(self, call):
        if call.fam.host:
            got = call.fam.call(self.obj, call.op, call.inputs)
        else:
            bufs, outs = self._buffers(call)
            self.t.cuda.synchronize()
            self._launch(call, bufs, 0)
            self.t.cuda.synchronize()
            got = self._down(bufs, outs)
        if self.seq.kind == "dec":
            self.cuts.append(self.obj.last_cut()[0])
        return got

    def prepare(self, calls):
        """every buffer of every call, uploaded / poisoned beforehand -> [(buffers, output shapes)]"""
        return [self._buffers(c) for c in calls]

    def enqueue(self, call, prepared, stream):
        self._launch(call, prepared[0], stream.cuda_stream)

    def fetch(self, prepared):
        return [self._down(bufs, outs) for bufs, outs in prepared]


class Recorded:
    """A backend that answers from outputs fetched earlier (a chain's), so that run() checks them call by call."""

    def __init__(self, outputs):
        self.outputs = iter(outputs)

    def run(self, call):
        return next(self.outputs)


# ---------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------
def census(seq):
    """What a sequence holds, for tests/test_call_axis_capi.py and profiles/call_axis_evidence.txt."""
    fams = families(seq.kind, seq.geom)
    names = list(fams)
    order = [c.op.family for c in seq.calls]
    pairs = {(a, b) for a, b in zip(order, order[1:])}
    streaming = [i for i, c in enumerate(seq.calls) if c.fam.streaming]
    lazy = {}
    for piece, what, i in seq.lazy_events:
        front = i < seq.prologue                            # in front of the walk: no call before it but the builders of other pieces
        between = not front and any(j < i for j in streaming) and any(j > i for j in streaming)
        lazy.setdefault(piece, []).append((what, i, "front" if front else "between" if between else "behind"))
    cut = {}
    for c in seq.calls:
        if "cut" in c.op.p:
            cut.setdefault(c.op.family, [0, 0])[0 if c.op.p["cut"] else 1] += 1
    behind_cut = sorted({b.op.family for a, b in zip(seq.calls, seq.calls[1:]) if a.op.p.get("cut")})
    return dict(names=names, order=order, missing_pairs=sorted({(a, b) for a in names for b in names} - pairs), lazy=lazy, cut=cut, behind_cut=behind_cut,
                lives=list(seq.model.n_lives), positions=list(seq.model.pos))


def pair_matrix(seq):
    """the pair matrix as text: row = the family in front, column = the family behind, the index of the call that makes the pair"""
    names = list(families(seq.kind, seq.geom))
    at = {}
    for a, b in zip(seq.calls, seq.calls[1:]):
        at.setdefault((a.op.family, b.op.family), b.op.i)
    lines = [f"{seq.kind} {seq.name} start {seq.start}: {len(seq.calls)} calls; columns in the rows' order"]
    for a in names:
        lines.append(f"  {a:28s} " + " ".join(f"{at.get((a, b), -1):4d}" for b in names))
    return lines
