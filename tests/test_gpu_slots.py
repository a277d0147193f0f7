"""Stream slots on the device (include/ulc_amd.h, "Stream slots"): subset calls, per-stream reset, save / load.

Every stream is checked against the oracle run on that stream ALONE (ulc_testlib.oracle_encode_debug / oracle_decode_stream):
a slot's blocks, concatenated over whatever calls it took part in, must be the oracle's uninterrupted encode / decode of the
PCM / blocks the slot was fed - byte for byte, d_bits, d_wc and the bit patterns of d_cplx and of the decoded samples.  The
device is never compared with itself, except where the property IS an identity (a subset call over every slot against the
plain call).  A `life` below is one stream in a slot: it starts at create, at a reset or at a load."""
import ctypes as C
import functools
import numpy as np
import pytest

from gpu_testlib import amd as _amd
import guarded_buffers as gb
from ulc_testlib import to_pcm16
from rates_testlib import mode_of
from seek_testlib import pack

pytestmark = pytest.mark.gpu

from call_axis_testlib import RATE, N_BLOCKS, VBR50, CBR64, TABLE, BIG, SMALL, _pcm, _oracle_enc, _oracle_blocks, _oracle_dec, _setting_fn, _Slots

A_PCM, A_PCM16, A_RATE, A_WORD, A_STATE = 16, 8, 8, 4, 16  # include/ulc_amd.h, "Caller buffers" and "Stream slots"


def _torch():
    import torch
    return torch


def _D(a):
    """numpy array -> device tensor (kept by the caller until its call has been synchronised)"""
    t = _torch()
    return t.from_numpy(np.ascontiguousarray(a)).to(t.device("cuda", 0))


def _Z(n, dtype):
    t = _torch()
    return t.zeros(n, dtype=getattr(t, np.dtype(dtype).name), device=t.device("cuda", 0))


def _sync():
    _torch().cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# inputs, oracle references and the lives model (_pcm, _oracle_*, _Slots): tests/call_axis_testlib.py, which extends them
# ---------------------------------------------------------------------------------------------------------------------
def _schedule(B, seed):
    """About ten calls: K over {1, 3, 8} (the window-control / transform pipeline's 1 / 3 / 4 launch shapes), n over {1, 5, 65,
    70} clipped to the object's slots (65 crosses the 64-stream group of the window-control kernels and the ragged end of the
    4-blocks-per-workgroup kernels), every value at least twice, in a seeded order; the list of each call a seeded shuffle."""
    rng = np.random.default_rng(seed)
    Ks = rng.permutation([1, 3, 8, 8, 1, 3, 8, 3, 1, 8])
    ns = rng.permutation([1, 5, 65, 70, 65, 5, 70, 1, 65, 70])
    return [(rng.permutation(B)[:min(int(n), B)].astype(np.int32), int(K)) for K, n in zip(Ks, ns)]


# ---------------------------------------------------------------------------------------------------------------------
# drivers: feed slots from their streams' PCM / blocks, keep what came back per life, compare with the oracle
# ---------------------------------------------------------------------------------------------------------------------
class EncDriver(_Slots):
    def __init__(self, geom, what=VBR50, sid=None):
        super().__init__(geom, sid)
        self.what, self.setting = what, _setting_fn(what)
        self.enc = _amd().BatchEncoder(self.B, self.ch, self.bs, RATE, self.maxK)
        self.slot = self.enc.slot

    def close(self):
        self.enc.close()

    def call(self, slots, K, kind="subset", bad=None, stream=0):
        """kind: subset | subset_pcm16 | plain | analyse_subset.  One call, synchronised, results kept."""
        slots = np.asarray(slots, np.int32)
        n = len(slots)
        rows = self.rows(slots, K, bad or {})
        x = np.stack([_pcm(self.bs, self.ch, sid)[a:a + K] for sid, a in rows])            # [n][K][bs][ch]
        pcm16 = kind == "subset_pcm16"
        d_slots, d_pcm = _D(slots), _D(np.rint(x * 32768.0).astype(np.int16) if pcm16 else x)
        d_out, d_bits, d_wc, d_cplx = _Z(n * K * self.slot, np.uint8), _Z(n * K, np.int32), _Z(n * K, np.int32), _Z(n * K, np.float32)
        table = self.what == "table"
        d_rate = _D(np.array([self.setting(sid) for sid, _ in rows], np.float32)) if table else None
        mode, p0, p1 = (0, 50.0, 0.0) if table else mode_of(self.what)
        P = lambda t: t.data_ptr()
        if kind == "plain":
            assert n == self.B and np.array_equal(slots, np.arange(self.B))
            if table:
                self.enc.encode_dev_rates(P(d_rate), P(d_pcm), K, P(d_out), P(d_bits), P(d_wc), P(d_cplx), stream=stream)
            else:
                self.enc.encode_dev(P(d_pcm), K, P(d_out), P(d_bits), P(d_wc), P(d_cplx), mode=mode, p0=p0, p1=p1, stream=stream)
        elif kind == "analyse_subset":
            self.enc.analyse_subset_dev(P(d_slots), n, P(d_pcm), K, P(d_wc), P(d_cplx), stream=stream)
        else:
            self.enc.encode_subset_dev(P(d_slots), n, P(d_pcm), K, P(d_out), P(d_bits), P(d_wc), P(d_cplx), mode=mode, p0=p0, p1=p1,
                                       d_rates=P(d_rate) if table else 0, stream=stream, pcm16=pcm16)
        _sync()
        out, bits = d_out.cpu().numpy().reshape(n, K, self.slot), d_bits.cpu().numpy().reshape(n, K)
        wc, cplx = d_wc.cpu().numpy().reshape(n, K), d_cplx.cpu().numpy().reshape(n, K)
        per_row = []
        for i in range(n):
            if kind == "analyse_subset":
                per_row.append([dict(bytes=None, bits=None, wc=int(wc[i, k]), cplx=cplx[i, k]) for k in range(K)])
            else:
                per_row.append([dict(bytes=out[i, k, :max(int(bits[i, k]), 0) // 8].copy(), bits=int(bits[i, k]), wc=int(wc[i, k]), cplx=cplx[i, k])
                                for k in range(K)])
        self.last = (out, bits, wc, cplx)
        return self.keep(slots, K, per_row)

    def compare(self, blocks, sid, origin, first, tag):
        """blocks: results of blocks first .. of the life that starts at block `origin` of stream sid"""
        ref = _oracle_enc(self.bs, self.ch, sid, origin, first + len(blocks), self.setting(sid))
        for j, b in enumerate(blocks):
            k, t = first + j, f"{tag}: stream {sid}, block {origin + first + j} (block {first + j} of its life)"
            assert b["wc"] == ref["wc"][k], f"{t}: WindowCtrl {b['wc']:#x} != {int(ref['wc'][k]):#x}"
            assert np.float32(b["cplx"]).tobytes() == ref["cplx"][k].tobytes(), f"{t}: BlockComplexity {b['cplx']} != {ref['cplx'][k]}"
            if b["bits"] is not None:
                assert b["bits"] == ref["bits"][k], f"{t}: size {b['bits']} != {int(ref['bits'][k])}"
                assert np.array_equal(b["bytes"], ref["out"][k, :b["bits"] // 8]), f"{t}: stream bytes differ"

    def check(self, tag):
        """every life of every slot against the oracle; -> number of decimated windows seen"""
        dec = 0
        for s in range(self.B):
            for life in self.lives[s]:
                if life["blocks"]:
                    self.compare(life["blocks"], life["sid"], life["origin"], life["first"], f"{tag}, slot {s}")
                    dec += sum(1 for b in life["blocks"] if b["wc"] & 8)
        return dec


class DecDriver(_Slots):
    def __init__(self, geom, sid=None):
        super().__init__(geom, sid)
        self.dec = _amd().BatchDecoder(self.B, self.ch, self.bs, self.maxK)
        self.slot = 2 * self.ch * self.bs + 16

    def close(self):
        self.dec.close()

    def call(self, slots, K, kind="subset", bad=None, stream=0):
        """kind: subset | subset_pcm16 | plain"""
        slots = np.asarray(slots, np.int32)
        n = len(slots)
        rows = self.rows(slots, K, bad or {})
        x = np.stack([_oracle_blocks(self.bs, self.ch, sid)[0][a:a + K] for sid, a in rows])      # [n][K][slot]
        pcm16 = kind == "subset_pcm16"
        d_slots, d_in = _D(slots), _D(x)
        d_pcm, d_bits = _Z(n * K * self.bs * self.ch, np.int16 if pcm16 else np.float32), _Z(n * K, np.int32)
        P = lambda t: t.data_ptr()
        if kind == "plain":
            assert n == self.B and np.array_equal(slots, np.arange(self.B))
            self.dec.decode_dev(P(d_in), self.slot, K, P(d_pcm), P(d_bits), stream=stream)
        else:
            self.dec.decode_subset_dev(P(d_slots), n, P(d_in), self.slot, K, P(d_pcm), P(d_bits), stream=stream, pcm16=pcm16)
        _sync()
        pcm, bits = d_pcm.cpu().numpy().reshape(n, K, self.bs, self.ch), d_bits.cpu().numpy().reshape(n, K)
        per_row = [[dict(pcm=pcm[i, k].copy(), bits=int(bits[i, k]), pcm16=pcm16) for k in range(K)] for i in range(n)]
        return self.keep(slots, K, per_row)

    def compare(self, blocks, key, first, tag):
        """blocks: results of blocks first .. of a life whose input was the oracle blocks `key` names (see _oracle_dec)"""
        ref, rbits = _oracle_dec(self.bs, self.ch, key)
        for j, b in enumerate(blocks):
            k, t = first + j, f"{tag}: blocks {key}, block {first + j} of its life"
            assert b["bits"] == rbits[k], f"{t}: bits {b['bits']} != {int(rbits[k])}"
            want = to_pcm16(ref[k]) if b["pcm16"] else ref[k]
            assert b["pcm"].tobytes() == want.tobytes(), f"{t}: {np.count_nonzero(b['pcm'] != want)} samples differ (noise included)"

    def check(self, tag):
        for s in range(self.B):
            for life in self.lives[s]:
                if life["blocks"]:
                    key = ((life["sid"], life["origin"], life["first"] + len(life["blocks"])),)
                    self.compare(life["blocks"], key, life["first"], f"{tag}, slot {s}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. schedules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [VBR50, CBR64, "table"], ids=["vbr", "cbr", "table"])
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["2048x2x70", "512x1x9"])
def test_encode_subset_schedule_equals_each_streams_own_oracle(geom, what):
    d = EncDriver(geom, what)
    sched = _schedule(d.B, 7)
    assert {K for _, K in sched} == {1, 3, 8} and {len(s) for s, _ in sched} == {min(n, d.B) for n in (1, 5, 65, 70)}
    for slots, K in sched:
        d.call(slots, K)
    decimated = d.check(f"schedule {what}")
    d.close()
    assert decimated >= 1, "no decimated window in the whole schedule: the inputs do not exercise window switching"
    assert max(d.pos) > 8 and min(d.pos) < max(d.pos), "the schedule must leave the slots at different positions"


# ---------------------------------------------------------------------------------------------------------------------
# 2. mixed with plain calls, 3. identity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [VBR50, "table"], ids=["vbr", "table"])
def test_subset_plain_and_analysis_subset_calls_mix(what):
    d = EncDriver(BIG, what)
    rng = np.random.default_rng(3)
    d.call(rng.permutation(d.B)[:65], 3)
    d.call(np.arange(d.B), 8, kind="plain")
    d.call(rng.permutation(d.B)[:5], 3, kind="analyse_subset")
    d.call(rng.permutation(d.B), 1)
    d.call(rng.permutation(d.B)[:65], 8)
    d.check(f"mixed {what}")
    d.close()


@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["2048x2x70", "512x1x9"])
def test_subset_over_every_slot_in_order_is_the_plain_call(geom):
    a, b = EncDriver(geom, CBR64), EncDriver(geom, CBR64)
    for K in (3, 8):
        a.call(np.arange(a.B), K)
        b.call(np.arange(b.B), K, kind="plain")
        (ao, ab, aw, ac), (bo, bb, bw, bc) = a.last, b.last
        assert np.array_equal(ab, bb) and np.array_equal(aw, bw) and ac.tobytes() == bc.tobytes()
        for s in range(a.B):
            for k in range(K):
                assert np.array_equal(ao[s, k, :ab[s, k] // 8], bo[s, k, :bb[s, k] // 8]), (s, k)
    a.check("identity, subset")
    b.check("identity, plain")
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. reset
# ---------------------------------------------------------------------------------------------------------------------
def test_reset_streams_restarts_the_listed_slots_only():
    d = EncDriver(BIG, VBR50)
    rng = np.random.default_rng(4)
    d.call(rng.permutation(d.B), 3)
    d.call(rng.permutation(d.B)[:65], 8)
    victims = np.array([1, 64, 69], np.int32)
    d_slots = _D(victims)
    d.enc.reset_streams_dev(d_slots.data_ptr(), len(victims))
    for s in victims:
        d.new_life(int(s))
    d.call(rng.permutation(d.B), 8)
    d.call(rng.permutation(d.B)[:65], 3)
    d.enc.reset_streams([5])                                # the host form
    d.new_life(5)
    d.call(rng.permutation(d.B), 1)
    d.check("reset")
    assert [len(d.lives[s]) for s in (1, 64, 69, 5, 0)] == [2, 2, 2, 2, 1]
    d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. save / load
# ---------------------------------------------------------------------------------------------------------------------
def _foreign_record(amd, make, nbytes):
    """A record saved by an object of another BlockSize, in a buffer of nbytes (this object's record size)"""
    other = make(1024)
    rec = other.save_streams([0])[0]
    other.close()
    out = np.zeros(nbytes, np.uint8)
    out[:min(nbytes, rec.size)] = rec[:nbytes]
    return out


def test_encoder_state_travels_between_objects():
    amd = _amd()
    bs, ch = BIG[0], BIG[1]
    a = EncDriver(BIG, CBR64)
    a.call([7, 2, 40], 3)
    rec = _Z(a.enc.state_bytes, np.uint8)
    d2 = _D(np.array([2], np.int32))
    a.enc.save_streams_dev(d2.data_ptr(), 1, rec.data_ptr())
    b = EncDriver((bs, ch, 9, 8), CBR64)
    b.call([5, 3], 1)                                       # slot 5 has a history of its own, which the load replaces
    d5 = _D(np.array([5], np.int32))
    b.enc.load_streams_dev(d5.data_ptr(), 1, rec.data_ptr())
    _sync()
    b.new_life(5, sid=2, origin=0, first=3)
    b.call([5, 0], 3)
    b.call([1, 5], 8)
    # a record of another BlockSize: refused by the host form, ignored by the device form - slot 5 goes on
    assert b.enc.state_bytes == a.enc.state_bytes and b.enc.state_bytes % 16 == 0
    bad = _foreign_record(amd, lambda q: amd.BatchEncoder(1, ch, q, RATE, 1), b.enc.state_bytes)
    with pytest.raises(amd.UlcError, match=r"\(-1\)"):
        b.enc.load_streams([5], bad)
    d_bad = _D(bad)
    b.enc.load_streams_dev(d5.data_ptr(), 1, d_bad.data_ptr())
    b.call([5, 2], 3)
    b.check("save / load, target")
    a.call([2, 7], 3)                                       # the source goes on as well
    a.check("save / load, source")
    # the host forms carry the same bytes
    assert np.array_equal(a.enc.save_streams([40])[0][:16].view(np.uint32), [amd_magic("E"), ch, bs, RATE])
    a.close(); b.close()


def amd_magic(kind):
    return int.from_bytes(b"UXS" + kind.encode(), "little")


# ---------------------------------------------------------------------------------------------------------------------
# 6. decoder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [BIG, SMALL], ids=["2048x2x70", "512x1x9"])
def test_decode_subset_schedule_equals_each_streams_own_oracle(geom):
    d = DecDriver(geom)
    for slots, K in _schedule(d.B, 11):
        d.call(slots, K)
    d.check("decode schedule")
    d.close()


def test_decoder_reset_streams_restarts_the_listed_slots_only():
    d = DecDriver(BIG)
    rng = np.random.default_rng(5)
    d.call(rng.permutation(d.B), 3)
    d.call(np.arange(d.B), 8, kind="plain")
    victims = np.array([1, 64, 69], np.int32)
    d_slots = _D(victims)
    d.dec.reset_streams_dev(d_slots.data_ptr(), len(victims))
    for s in victims:
        d.new_life(int(s))
    d.call(rng.permutation(d.B)[:65], 8)
    d.dec.reset_streams([5])
    d.new_life(5)
    d.call(rng.permutation(d.B), 3)
    d.check("decoder reset")
    d.close()


def test_decoder_state_travels_between_objects():
    amd = _amd()
    bs, ch = BIG[0], BIG[1]
    a = DecDriver(BIG)
    a.call([7, 2, 40], 3)
    rec = _Z(a.dec.state_bytes, np.uint8)
    d2 = _D(np.array([2], np.int32))
    a.dec.save_streams_dev(d2.data_ptr(), 1, rec.data_ptr())
    b = DecDriver((bs, ch, 9, 8))
    b.call([5, 3], 1)
    d5 = _D(np.array([5], np.int32))
    b.dec.load_streams_dev(d5.data_ptr(), 1, rec.data_ptr())
    _sync()
    b.new_life(5, sid=2, origin=0, first=3)
    b.call([5, 0], 3)
    bad = _foreign_record(amd, lambda q: amd.BatchDecoder(1, ch, q, 1), b.dec.state_bytes)
    with pytest.raises(amd.UlcError, match=r"\(-1\)"):
        b.dec.load_streams([5], bad)
    d_bad = _D(bad)
    b.dec.load_streams_dev(d5.data_ptr(), 1, d_bad.data_ptr())
    b.call([1, 5], 8)
    b.check("decoder save / load, target")
    a.call([2, 7], 3)
    a.check("decoder save / load, source")
    assert np.array_equal(a.dec.save_streams([40])[0][:16].view(np.uint32), [amd_magic("D"), ch, bs, 0])
    a.close(); b.close()


def test_decode_subset_with_a_cut_synthesis_keeps_its_own_state_sets():
    """Few long streams: the synthesis of the subset call takes an even cut, whose result lands in the second set of the compact
    state; the scatter must read that set, and the object's own sets must stay where they are for the next call."""
    d = DecDriver((2048, 2, 8, 24))
    d.call(np.arange(8), 1, kind="plain")                   # every slot has state of its own in the object's first set
    d.call([6, 1], 24)
    g, full, resident = d.dec.last_cut()
    assert resident > 0 and g > 0, f"the synthesis of a 2-stream, 24-block call was not cut (workgroups {g}, resident {resident})"
    d.call([1, 6], 16)
    g2, _, _ = d.dec.last_cut()
    assert g2 > 0
    d.call(np.arange(8), 1, kind="plain")                   # the other slots are where the first call left them
    d.call([6, 3], 4)
    d.check("cut synthesis")
    d.close()


def test_packed_read_position_travels_with_a_saved_slot():
    """decode_packed_dev on a slot that was saved in one decoder and loaded into another continues behind the blocks the first
    decoder had consumed; a subset call in between moves no read position."""
    bs, ch, B, K = 2048, 2, 3, 3
    a, b = DecDriver((bs, ch, B, 8)), DecDriver((bs, ch, B, 8))
    payload, nbytes = pack([(_oracle_blocks(bs, ch, s)[0][:12], _oracle_blocks(bs, ch, s)[1][:12]) for s in range(B)])
    d_pay, d_n = _D(payload), _D(nbytes)
    d_pcm, d_bits = _Z(B * K * bs * ch, np.float32), _Z(B * K, np.int32)
    a.dec.decode_packed_dev(d_pay.data_ptr(), payload.shape[1], d_n.data_ptr(), K, d_pcm.data_ptr(), d_bits.data_ptr())
    _sync()
    for s in range(B):
        assert d_pcm.cpu().numpy().reshape(B, K, bs, ch)[s].tobytes() == _oracle_dec(bs, ch, ((s, 0, K),))[0].tobytes()
    rec = _Z(a.dec.state_bytes, np.uint8)
    d1, d2, d0 = _D(np.array([1], np.int32)), _D(np.array([2], np.int32)), _D(np.array([0], np.int32))
    a.dec.save_streams_dev(d1.data_ptr(), 1, rec.data_ptr())
    # target: stream 1's payload in row 2, the others fresh; slot 0 first takes a subset call of two slot-form blocks
    pay_b = payload[[0, 0, 1]].copy()
    n_b = nbytes[[0, 0, 1]].copy()
    b.sid = [0, 0, 1]
    b.lives = [[dict(sid=b.sid[s], origin=0, first=0, blocks=[])] for s in range(B)]
    b.dec.load_streams_dev(d2.data_ptr(), 1, rec.data_ptr())
    b.call([0], 2)
    d_pay_b, d_n_b = _D(pay_b), _D(n_b)
    b.dec.decode_packed_dev(d_pay_b.data_ptr(), pay_b.shape[1], d_n_b.data_ptr(), K, d_pcm.data_ptr(), d_bits.data_ptr())
    _sync()
    got, gbits = d_pcm.cpu().numpy().reshape(B, K, bs, ch), d_bits.cpu().numpy().reshape(B, K)
    want = [_oracle_dec(bs, ch, ((0, 0, 2), (0, 0, K))),    # slot 0: two blocks in slot form, then the payload from its start
            _oracle_dec(bs, ch, ((0, 0, K),)),              # slot 1: fresh
            _oracle_dec(bs, ch, ((1, 0, 2 * K),))]          # slot 2: stream 1 continued behind the K blocks decoder a consumed
    for s, (wp, wb) in enumerate(want):
        assert np.array_equal(gbits[s], wb[-K:]), (s, gbits[s], wb[-K:])
        assert got[s].tobytes() == wp[-K:].tobytes(), f"slot {s}: packed continuation differs from the oracle"
    b.check("packed, subset call")
    a.close(); b.close()


def test_decode_subset_pcm16():
    d = DecDriver(BIG)
    rng = np.random.default_rng(6)
    d.call(rng.permutation(d.B)[:65], 3, kind="subset_pcm16")
    d.call(rng.permutation(d.B)[:5], 8, kind="subset_pcm16")
    d.call(rng.permutation(d.B), 1)
    d.check("pcm16")
    d.close()


def test_encode_subset_pcm16():
    d = EncDriver(BIG, VBR50)
    rng = np.random.default_rng(8)
    d.call(rng.permutation(d.B)[:65], 3, kind="subset_pcm16")
    d.call(rng.permutation(d.B)[:5], 8)
    d.check("encode pcm16")
    d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. lists
# ---------------------------------------------------------------------------------------------------------------------
def test_host_forms_refuse_bad_lists_and_leave_the_object_untouched():
    amd = _amd()
    e, d = EncDriver(SMALL, VBR50), DecDriver(SMALL)
    e.call([3, 0, 8], 3)
    d.call([3, 0, 8], 3)
    x = np.zeros((2, 3 * e.bs, e.ch), np.float32)
    blk = np.zeros((2, 3, d.slot), np.uint8)
    for lst in ([3, 3], [-1, 0], [0, e.B]):
        for call in (lambda: e.enc.encode_subset(lst, x), lambda: e.enc.reset_streams(lst), lambda: e.enc.save_streams(lst),
                     lambda: e.enc.load_streams(lst, np.zeros((2, e.enc.state_bytes), np.uint8)),
                     lambda: d.dec.decode_subset(lst, blk), lambda: d.dec.reset_streams(lst), lambda: d.dec.save_streams(lst),
                     lambda: d.dec.load_streams(lst, np.zeros((2, d.dec.state_bytes), np.uint8))):
            with pytest.raises(amd.UlcError, match=r"\(-1\)"):
                call()
    e.call([0, 3, 5], 3)
    d.call([0, 3, 5], 3)
    # the host subset forms themselves, on the same objects
    rows = [(e.sid[s], e.pos[s]) for s in (8, 3)]
    out, bits, wc, cplx = e.enc.encode_subset([8, 3], np.stack([_pcm(e.bs, e.ch, sid)[a:a + 2].reshape(2 * e.bs, e.ch) for sid, a in rows]))
    e.keep([8, 3], 2, [[dict(bytes=out[i, k, :bits[i, k] // 8].copy(), bits=int(bits[i, k]), wc=int(wc[i, k]), cplx=cplx[i, k]) for k in range(2)] for i in range(2)])
    rows = [(d.sid[s], d.pos[s]) for s in (8, 3)]
    pcm, bits = d.dec.decode_subset([8, 3], np.stack([_oracle_blocks(d.bs, d.ch, sid)[0][a:a + 2] for sid, a in rows]))
    pcm = pcm.reshape(2, 2, d.bs, d.ch)
    d.keep([8, 3], 2, [[dict(pcm=pcm[i, k].copy(), bits=int(bits[i, k]), pcm16=False) for k in range(2)] for i in range(2)])
    e.call([8, 3, 0], 1)
    d.call([8, 3, 0], 1)
    e.check("bad host lists")
    d.check("bad host lists")
    e.close(); d.close()


def test_device_forms_run_an_out_of_range_entry_from_a_fresh_state_and_drop_it():
    geom = (2048, 2, 9, 8)
    e, d = EncDriver(geom, CBR64), DecDriver(geom)
    for drv in (e, d):
        drv.call([3, 0], 3)
        for badslot in (drv.B, -1):
            extra = drv.call([3, badslot, 0], 3, bad={1: 20})
            if drv is e:
                e.compare(extra[1], 20, 0, 0, f"row of entry {badslot}")
            else:
                d.compare(extra[1], ((20, 0, 3),), 0, f"row of entry {badslot}")
        drv.call([0, 3, 8], 3)
    # save writes a fresh-state record for it, reset and load skip it
    fresh = _amd().BatchEncoder(1, 2, 2048, RATE, 1)
    want = fresh.save_streams([0])[0]
    fresh.close()
    lst = _D(np.array([e.B, 3], np.int32))
    rec = _Z(2 * e.enc.state_bytes, np.uint8)
    e.enc.save_streams_dev(lst.data_ptr(), 2, rec.data_ptr())
    e.enc.reset_streams_dev(lst.data_ptr(), 1)
    e.enc.load_streams_dev(lst.data_ptr(), 1, rec.data_ptr())
    _sync()
    got = rec.cpu().numpy().reshape(2, -1)
    assert np.array_equal(got[0], want) and not np.array_equal(got[1], want)
    e.call([3, 0], 3)
    e.check("out-of-range entry")
    d.check("out-of-range entry")
    e.close(); d.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. buffer contract of the new _dev entries: poisoned buffers between guards, stream order, misaligned pointers
# ---------------------------------------------------------------------------------------------------------------------
CG = (2048, 2, 9, 5)                                       # geometry of the contract cases; calls of K = 3 < maxBlocksPerCall
CK, CSLOTS = 3, [7, 2, 8, 0]


def _guarded_encode(kind):
    """one encode / analyse subset call with every buffer carved from a poisoned arena -> (driver, arena, fetched outputs)"""
    bs, ch, B, maxK = CG
    e = EncDriver(CG, "table" if kind == "subset" else VBR50)
    e.call([2, 0, 5], 2)                                    # carried state
    n, K, slot = len(CSLOTS), CK, e.slot
    pcm16, analyse = kind == "subset_pcm16", kind == "analyse_subset"
    row = bs * ch * (2 if pcm16 else 4)
    specs = [dict(name="d_slots", nbytes=4 * n, align=A_WORD, role="in", guard=4 * B),
             dict(name="d_pcm", nbytes=n * K * row, align=A_PCM16 if pcm16 else A_PCM, role="in", guard=B * maxK * row, row=row, rows_per_stream=K),
             dict(name="d_wc", nbytes=4 * n * K, align=A_WORD, role="out", guard=4 * B * maxK, row=4, rows_per_stream=K),
             dict(name="d_cplx", nbytes=4 * n * K, align=A_WORD, role="out", guard=4 * B * maxK, row=4, rows_per_stream=K)]
    if not analyse:
        specs += [dict(name="d_out", nbytes=n * K * slot, align=1, role="out", guard=B * maxK * slot, row=slot, rows_per_stream=K),
                  dict(name="d_bits", nbytes=4 * n * K, align=A_WORD, role="out", guard=4 * B * maxK, row=4, rows_per_stream=K)]
    if kind == "subset":
        specs.append(dict(name="d_rate", nbytes=8 * n, align=A_RATE, role="in", guard=8 * B, row=8))
    a = gb.build(_torch().device("cuda", 0), specs)
    rows = e.rows(CSLOTS, K, {})
    x = np.stack([_pcm(bs, ch, sid)[p:p + K] for sid, p in rows])
    a.load("d_slots", np.array(CSLOTS, np.int32))
    a.load("d_pcm", np.rint(x * 32768.0).astype(np.int16) if pcm16 else x)
    if kind == "subset":
        a.load("d_rate", np.array([e.setting(sid) for sid, _ in rows], np.float32))
    return e, a


def _kept_rows(e, a, analyse):
    n, K = len(CSLOTS), CK
    wc, cplx = a.fetch("d_wc", np.int32).reshape(n, K), a.fetch("d_cplx", np.float32).reshape(n, K)
    if analyse:
        return [[dict(bytes=None, bits=None, wc=int(wc[i, k]), cplx=cplx[i, k]) for k in range(K)] for i in range(n)]
    out, bits = a.fetch("d_out").reshape(n, K, e.slot), a.fetch("d_bits", np.int32).reshape(n, K)
    return [[dict(bytes=out[i, k, :max(int(bits[i, k]), 0) // 8].copy(), bits=int(bits[i, k]), wc=int(wc[i, k]), cplx=cplx[i, k]) for k in range(K)]
            for i in range(n)]


@pytest.mark.parametrize("kind", ["subset", "subset_pcm16", "analyse_subset"])
def test_encoder_subset_entries_on_poisoned_guarded_buffers(kind):
    e, a = _guarded_encode(kind)
    p, n = a.ptr, len(CSLOTS)
    if kind == "analyse_subset":
        e.enc.analyse_subset_dev(p("d_slots"), n, p("d_pcm"), CK, p("d_wc"), p("d_cplx"))
    else:
        e.enc.encode_subset_dev(p("d_slots"), n, p("d_pcm"), CK, p("d_out"), p("d_bits"), p("d_wc"), p("d_cplx"),
                                d_rates=p("d_rate") if kind == "subset" else 0, pcm16=kind == "subset_pcm16")
    _sync()
    a.check()
    e.keep(CSLOTS, CK, _kept_rows(e, a, kind == "analyse_subset"))       # over poison: every element is the oracle's, so every one was written
    e.call([0, 7, 3], 2)
    e.check(f"guarded {kind}")
    e.close()


@pytest.mark.parametrize("pcm16", [False, True], ids=["f32", "pcm16"])
def test_decoder_subset_entries_on_poisoned_guarded_buffers(pcm16):
    bs, ch, B, maxK = CG
    d = DecDriver(CG)
    d.call([2, 0, 5], 2)
    n, K, slot = len(CSLOTS), CK, d.slot
    row = bs * ch * (2 if pcm16 else 4)
    a = gb.build(_torch().device("cuda", 0), [
        dict(name="d_slots", nbytes=4 * n, align=A_WORD, role="in", guard=4 * B),
        dict(name="d_in", nbytes=n * K * slot, align=1, role="in", guard=B * maxK * slot, row=slot, rows_per_stream=K),
        dict(name="d_pcm", nbytes=n * K * row, align=A_PCM16 if pcm16 else A_PCM, role="out", guard=B * maxK * row, row=row, rows_per_stream=K),
        dict(name="d_bits", nbytes=4 * n * K, align=A_WORD, role="out", guard=4 * B * maxK, row=4, rows_per_stream=K)])
    rows = d.rows(CSLOTS, K, {})
    a.load("d_slots", np.array(CSLOTS, np.int32))
    a.load("d_in", np.stack([_oracle_blocks(bs, ch, sid)[0][p:p + K] for sid, p in rows]))
    p = a.ptr
    d.dec.decode_subset_dev(p("d_slots"), n, p("d_in"), slot, K, p("d_pcm"), p("d_bits"), pcm16=pcm16)
    _sync()
    a.check()
    pcm, bits = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, K, bs, ch), a.fetch("d_bits", np.int32).reshape(n, K)
    d.keep(CSLOTS, K, [[dict(pcm=pcm[i, k].copy(), bits=int(bits[i, k]), pcm16=pcm16) for k in range(K)] for i in range(n)])
    d.call([0, 7, 3], 2)
    d.check("guarded decode subset")
    d.close()


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_reset_save_load_entries_on_poisoned_guarded_buffers(kind):
    """save writes all n records in full (the same bytes over poison as over zeros), header and input history as stated; load
    and reset read their list and records only; the loaded and the reset slots continue as the oracle says."""
    bs, ch, B, maxK = CG
    drv = EncDriver(CG, VBR50) if kind == "encoder" else DecDriver(CG)
    obj = drv.enc if kind == "encoder" else drv.dec
    drv.call([7, 2, 8, 0, 4], 3)
    n, sb = len(CSLOTS), obj.state_bytes
    assert sb % 16 == 0
    a = gb.build(_torch().device("cuda", 0), [
        dict(name="d_slots", nbytes=4 * n, align=A_WORD, role="in", guard=4 * B),
        dict(name="d_state", nbytes=n * sb, align=A_STATE, role="out", guard=B * sb, row=sb)])
    a.load("d_slots", np.array(CSLOTS, np.int32))
    obj.save_streams_dev(a.ptr("d_slots"), n, a.ptr("d_state"))
    plain = _Z(n * sb, np.uint8)
    obj.save_streams_dev(a.ptr("d_slots"), n, plain.data_ptr())
    _sync()
    a.check()
    rec = a.fetch("d_state").reshape(n, sb)
    assert np.array_equal(rec, plain.cpu().numpy().reshape(n, sb)), "a saved record keeps bytes of the buffer it was written into"
    assert np.array_equal(rec, obj.save_streams(CSLOTS)), "host and device save differ"
    for i, s in enumerate(CSLOTS):
        assert np.array_equal(rec[i, :16].view(np.uint32), [amd_magic("E" if kind == "encoder" else "D"), ch, bs, RATE if kind == "encoder" else 0])
        if kind == "encoder":                               # the two blocks of input history
            assert rec[i, 16:16 + 2 * bs * ch * 4].tobytes() == _pcm(bs, ch, drv.sid[s])[drv.pos[s] - 2:drv.pos[s]].tobytes()
    # load the records into other slots of a second object (in: nothing of the caller's is written), reset two of them
    other = EncDriver(CG, VBR50) if kind == "encoder" else DecDriver(CG)
    oobj = other.enc if kind == "encoder" else other.dec
    other.call([1, 3, 5], 1)
    targets = [3, 6, 1, 5]
    b = gb.build(_torch().device("cuda", 0), [
        dict(name="d_slots", nbytes=4 * n, align=A_WORD, role="in", guard=4 * B),
        dict(name="d_state", nbytes=n * sb, align=A_STATE, role="in", guard=B * sb, row=sb),
        dict(name="d_reset", nbytes=8, align=A_WORD, role="in", guard=4 * B)])
    b.load("d_slots", np.array(targets, np.int32))
    b.load("d_state", rec)
    b.load("d_reset", np.array([6, 0], np.int32))
    oobj.load_streams_dev(b.ptr("d_slots"), n, b.ptr("d_state"))
    oobj.reset_streams_dev(b.ptr("d_reset"), 2)
    _sync()
    b.check()
    for t, s in zip(targets, CSLOTS):
        other.new_life(t, sid=drv.sid[s], origin=0, first=drv.pos[s])
    other.new_life(6, sid=6, origin=0)
    other.new_life(0, sid=0, origin=0)
    other.call([6, 3, 1, 5, 0], 3)
    other.check(f"guarded load / reset, {kind}")
    drv.check(f"guarded save, {kind}")
    drv.close(); other.close()


def test_misaligned_slot_lists_and_records_are_refused_before_any_device_work():
    amd = _amd()
    e, d = EncDriver(SMALL, VBR50), DecDriver(SMALL)
    e.call([3, 0], 3)
    d.call([3, 0], 3)
    buf = _Z(1 << 20, np.uint8)
    base = (buf.data_ptr() + 255) & ~255
    lst, big = base + 4096, base + 65536
    for obj in (e.enc, d.dec):
        for call in (lambda: obj.reset_streams_dev(lst + 2, 1), lambda: obj.save_streams_dev(lst + 1, 1, big),
                     lambda: obj.save_streams_dev(lst, 1, big + 8), lambda: obj.load_streams_dev(lst + 2, 1, big),
                     lambda: obj.load_streams_dev(lst, 1, big + 4)):
            with pytest.raises(amd.UlcError, match=r"\(-1\)"):
                call()
    for bad in (lst + 2, lst + 1):
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            e.enc.encode_subset_dev(bad, 1, big, 1, big, big, big, big)
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            e.enc.analyse_subset_dev(bad, 1, big, 1, big, big)
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            d.dec.decode_subset_dev(bad, 1, big, 64, 1, big, big)
    for n in (0, e.B + 1):                                 # n outside 1 .. nStreams
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            e.enc.encode_subset_dev(lst, n, big, 1, big, big, big, big)
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            d.dec.decode_subset_dev(lst, n, big, 64, 1, big, big)
    e.call([0, 3, 5], 3)
    d.call([0, 3, 5], 3)
    e.check("after refused calls")
    d.check("after refused calls")
    e.close(); d.close()


def test_work_enqueued_behind_a_slot_call_sees_its_results_without_synchronisation():
    """On a stream of the caller's: subset encode, a copy of its outputs, the input overwritten, the state saved, a copy of the
    record, the slots reset - nothing waits in between; the copies hold the call's results."""
    t = _torch()
    bs, ch, B, maxK = CG
    e, d = EncDriver(CG, VBR50), DecDriver(CG)
    e.call([2, 0, 5], 2)
    d.call([2, 0, 5], 2)
    n, K = len(CSLOTS), CK
    rows_e, rows_d = e.rows(CSLOTS, K, {}), d.rows(CSLOTS, K, {})
    d_slots = _D(np.array(CSLOTS, np.int32))
    d_pcm = _D(np.stack([_pcm(bs, ch, sid)[p:p + K] for sid, p in rows_e]))
    d_in = _D(np.stack([_oracle_blocks(bs, ch, sid)[0][p:p + K] for sid, p in rows_d]))
    d_out, d_bits, d_wc, d_cplx = _Z(n * K * e.slot, np.uint8), _Z(n * K, np.int32), _Z(n * K, np.int32), _Z(n * K, np.float32)
    o_pcm, o_bits = _Z(n * K * bs * ch, np.float32), _Z(n * K, np.int32)
    rec_e, rec_d = _Z(n * e.enc.state_bytes, np.uint8), _Z(n * d.dec.state_bytes, np.uint8)
    _sync()
    st = t.cuda.Stream()
    P = lambda x: x.data_ptr()
    with t.cuda.stream(st):
        e.enc.encode_subset_dev(P(d_slots), n, P(d_pcm), K, P(d_out), P(d_bits), P(d_wc), P(d_cplx), stream=st.cuda_stream)
        c_out, c_bits, c_wc, c_cplx = d_out.clone(), d_bits.clone(), d_wc.clone(), d_cplx.clone()
        d_pcm.fill_(0.25); d_out.fill_(7); d_bits.fill_(-5)
        e.enc.save_streams_dev(P(d_slots), n, P(rec_e), stream=st.cuda_stream)
        c_rec_e = rec_e.clone()
        rec_e.fill_(9)
        e.enc.reset_streams_dev(P(d_slots), n, stream=st.cuda_stream)
        d.dec.decode_subset_dev(P(d_slots), n, P(d_in), d.slot, K, P(o_pcm), P(o_bits), stream=st.cuda_stream)
        c_pcm, c_obits = o_pcm.clone(), o_bits.clone()
        d_in.fill_(0); o_pcm.fill_(1.0)
        d.dec.save_streams_dev(P(d_slots), n, P(rec_d), stream=st.cuda_stream)
        c_rec_d = rec_d.clone()
        d.dec.reset_streams_dev(P(d_slots), n, stream=st.cuda_stream)
    st.synchronize()
    _sync()
    out, bits = c_out.cpu().numpy().reshape(n, K, e.slot), c_bits.cpu().numpy().reshape(n, K)
    wc, cplx = c_wc.cpu().numpy().reshape(n, K), c_cplx.cpu().numpy().reshape(n, K)
    e.keep(CSLOTS, K, [[dict(bytes=out[i, k, :max(int(bits[i, k]), 0) // 8].copy(), bits=int(bits[i, k]), wc=int(wc[i, k]), cplx=cplx[i, k]) for k in range(K)]
                       for i in range(n)])
    pcm, obits = c_pcm.cpu().numpy().reshape(n, K, bs, ch), c_obits.cpu().numpy().reshape(n, K)
    d.keep(CSLOTS, K, [[dict(pcm=pcm[i, k].copy(), bits=int(obits[i, k]), pcm16=False) for k in range(K)] for i in range(n)])
    # the records were saved behind the calls and in front of the resets: loaded back, the slots go on; slot 2's reset stays
    keep = [i for i, s in enumerate(CSLOTS) if s != 2]
    lst = _D(np.array([CSLOTS[i] for i in keep], np.int32))
    re = _D(c_rec_e.cpu().numpy().reshape(n, -1)[keep])
    rd = _D(c_rec_d.cpu().numpy().reshape(n, -1)[keep])
    e.enc.load_streams_dev(P(lst), len(keep), P(re))
    d.dec.load_streams_dev(P(lst), len(keep), P(rd))
    _sync()
    e.new_life(2)
    d.new_life(2)
    e.call([2, 7, 8, 0], 3)
    d.call([2, 7, 8, 0], 3)
    e.check("stream order")
    d.check("stream order")
    e.close(); d.close()
