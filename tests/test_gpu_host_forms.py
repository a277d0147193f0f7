"""The host-pointer forms' own logic (ulcx_api.cpp: checks, staging, ownership), not the kernels': a refused call changes
nothing, staging that grows or is replaced keeps working, a replaced payload drops its index.  One small geometry - three
stereo streams, BlockSize 256, four blocks a call at most - since the geometry only has to be valid."""
import ctypes as C
import numpy as np
import pytest

from gpu_testlib import amd
from ulc_testlib import synth_pcm
from seek_testlib import pack

pytestmark = pytest.mark.gpu

B, CH, BS, RATE, MAXK = 3, 2, 256, 44100, 4
T = 5                                                      # blocks of signal per stream: calls of 2 and 3
NAN = float("nan")


def p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


@pytest.fixture(scope="module")
def pcm():
    x = np.stack([synth_pcm(s, T * BS, CH, RATE, transient=True, seed=23) for s in range(B)])
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def blocks(pcm):
    """The signal encoded at two qualities, in calls of 2 and 3 blocks: {quality: (slots uint8 [B][T][slot], bits [B][T])}"""
    r = {}
    enc = amd().BatchEncoder(B, CH, BS, RATE, MAXK)
    for q in (50.0, 20.0):
        enc.reset()
        o0, b0, _, _ = enc.encode(pcm[:, :2 * BS], 0, q)
        o1, b1, _, _ = enc.encode(pcm[:, 2 * BS:], 0, q)
        out, bits = np.concatenate([o0, o1], axis=1), np.concatenate([b0, b1], axis=1)
        assert (bits > 0).all() and (bits % 8 == 0).all()
        for k in range(T):                                 # (the rest of a slot is not defined: read a slot through its size)
            for s in range(B):
                out[s, k, bits[s, k] // 8:] = 0
        out.setflags(write=False), bits.setflags(write=False)
        r[q] = (out, bits)
    enc.close()
    assert not np.array_equal(r[50.0][1], r[20.0][1])
    return r


def refused(rc, name):
    msg = amd().lib().ulcx_last_error().decode()
    assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)
    return msg


def same_encoding(a, b):
    """(out, bits, wc, cplx) of two calls: sizes, window codes and complexities equal, and every block byte for byte"""
    (oa, ba, wa, ca), (ob, bb, wb, cb) = a, b
    assert np.array_equal(ba, bb) and np.array_equal(wa, wb) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
    for idx in np.ndindex(ba.shape):
        n = int(ba[idx]) // 8
        assert n > 0 and np.array_equal(oa[idx][:n], ob[idx][:n]), idx


def consumed(dbits, sizes):
    """The decoder counts the nybbles it read, the encoder's size is that rounded up to whole bytes"""
    return np.array_equal((np.asarray(dbits) + 7) // 8 * 8, sizes)


def test_refused_host_calls_leave_the_state_alone(pcm, blocks):
    u = amd()
    L = u.lib()
    # ---- encoder: A and B encode two blocks, A is refused seven times, both encode the next three
    A, Bn = u.BatchEncoder(B, CH, BS, RATE, MAXK), u.BatchEncoder(B, CH, BS, RATE, MAXK)
    same_encoding(A.encode(pcm[:, :2 * BS], 0, 50.0), Bn.encode(pcm[:, :2 * BS], 0, 50.0))
    big = np.ascontiguousarray(np.tile(pcm, (1, 2, 1))[:, :(MAXK + 1) * BS])          # room for the call that asks for too much
    out = np.zeros((2, B, MAXK + 1, A.slot), np.uint8)                                # (two rungs' worth)
    bits, wc, cplx = np.zeros((2, B, MAXK + 1), np.int32), np.zeros((B, MAXK + 1), np.int32), np.zeros((B, MAXK + 1), np.float32)
    f32, i32, u8 = C.c_float, C.c_int32, C.c_uint8
    o = (p(out, u8), p(bits, i32), p(wc, i32), p(cplx, f32))
    refused(L.ulcx_encode_host(A.h, 0, 50.0, 0.0, p(big, f32), MAXK + 1, *o), "ulcx_encode_host")
    refused(L.ulcx_encode_host(A.h, 7, 50.0, 0.0, p(big, f32), 3, *o), "ulcx_encode_host")
    rates = np.array([[-50.0, 0.0], [0.0, 0.0], [64.0, 0.0]], np.float32)
    refused(L.ulcx_encode_host_rates(A.h, p(rates, f32), p(big, f32), 3, *o), "ulcx_encode_host_rates")
    rungs = (u.Rung * 2)()
    rungs[0].mode, rungs[0].param0 = 0, 50.0
    rungs[1].mode, rungs[1].param0, rungs[1].reserved = 1, 64.0, 1
    refused(L.ulcx_encode_host_ladder(A.h, rungs, 2, p(big, f32), 3, *o), "ulcx_encode_host_ladder")
    rungs[1].reserved, rungs[1].param0 = 0, NAN
    refused(L.ulcx_encode_host_ladder(A.h, rungs, 2, p(big, f32), 3, *o), "ulcx_encode_host_ladder")
    twice = np.array([0, 0], np.int32)
    msg = refused(L.ulcx_encode_host_subset(A.h, p(twice, i32), 2, 0, 50.0, 0.0, None, p(big, f32), 3, *o), "ulcx_encode_host_subset")
    assert "listed twice" in msg
    refused(L.ulcx_analyse_host(A.h, p(big, f32), 3, None, None), "ulcx_analyse_host")
    same_encoding(A.encode(pcm[:, 2 * BS:], 0, 50.0), Bn.encode(pcm[:, 2 * BS:], 0, 50.0))
    A.close(), Bn.close()

    # ---- decoder: the same, with the payload both objects need for the resident range call uploaded (that rewinds them) first
    slots, sizes = blocks[50.0]
    pay, pay_bytes = pack([(slots[s], sizes[s]) for s in range(B)])
    A, Bn = u.BatchDecoder(B, CH, BS, MAXK), u.BatchDecoder(B, CH, BS, MAXK)
    hp, hb = np.zeros((B, MAXK * BS, CH), np.float32), np.zeros((B, MAXK), np.int32)
    msg = refused(L.ulcx_decode_resident_host(A.h, 2, p(hp, f32), p(hb, i32)), "ulcx_decode_resident_host")
    assert "no payload" in msg
    index, count = A.index_packed(pay, pay_bytes, T)
    assert (count == T).all()
    for d in (A, Bn):
        d.upload_payload(pay, pay_bytes)
        assert (d.index_resident(T) == T).all()
    ra, rb = A.decode(slots[:, :2]), Bn.decode(slots[:, :2])
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and consumed(ra[1], sizes[:, :2])
    refused(L.ulcx_decode_host(A.h, p(slots, u8), 0, 2, p(hp, f32), p(hb, i32)), "ulcx_decode_host")
    outside = np.array([0, B], np.int32)
    msg = refused(L.ulcx_decode_host_subset(A.h, p(outside, i32), 2, p(slots, u8), slots.shape[2], 2, p(hp, f32), p(hb, i32)), "ulcx_decode_host_subset")
    assert "outside" in msg
    first = np.array([1, -1, 0], np.int32)
    msg = refused(L.ulcx_decode_range_host(A.h, p(pay, u8), pay.shape[1], p(pay_bytes, i32), index.ctypes.data, index.shape[1], p(count, i32),
                                           p(first, i32), 2, p(hp, f32), p(hb, i32)), "ulcx_decode_range_host")
    assert "starts at block -1" in msg
    msg = refused(L.ulcx_decode_resident_range_host(A.h, p(first, i32), 2, p(hp, f32), p(hb, i32)), "ulcx_decode_resident_range_host")
    assert "starts at block -1" in msg
    ra, rb = A.decode(slots[:, 2:]), Bn.decode(slots[:, 2:])
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and consumed(ra[1], sizes[:, 2:])
    assert np.abs(ra[0]).max() > 0.01
    A.close(), Bn.close()


def test_staging_that_grows(pcm, blocks):
    u = amd()
    # ---- the decoder's input slots: a tight slotBytes first, the encoder's full slot after it
    slots, sizes = blocks[50.0]
    K = 3
    tight = int(sizes[:, :K].max()) // 8
    assert tight < slots.shape[2]
    fresh = u.BatchDecoder(B, CH, BS, MAXK)
    want = fresh.decode(slots[:, :K])
    fresh.close()
    assert consumed(want[1], sizes[:, :K]) and np.abs(want[0]).max() > 0.01
    d = u.BatchDecoder(B, CH, BS, MAXK)
    for width in (tight, slots.shape[2]):
        got = d.decode(slots[:, :K, :width])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), width
        d.reset()
    d.close()

    # ---- the same buffer under a single-block decoder: its captured sequence must follow the buffer (blocks 0 and 2 through
    # the single-block call, block 1 through a host call whose slots are wider than the single-block path's)
    one = slots[:1]
    ref = u.BatchDecoder(1, CH, BS, 1)
    seq = [ref.decode(one[:, k:k + 1])[0] for k in range(3)]
    ref.close()
    d = u.BatchDecoder(1, CH, BS, 1)
    L = u.lib()
    L.ulcx_decode_block1.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    wide = np.zeros((1, 1, one.shape[2] + 256), np.uint8)
    wide[:, :, :one.shape[2]] = one[:, 1:2]
    for k in range(3):
        if k == 1:
            got = d.decode(wide)[0]
        else:
            got, nb = np.zeros((1, BS, CH), np.float32), C.c_int32(0)
            blk = np.ascontiguousarray(one[0, k])
            assert L.ulcx_decode_block1(d.h, blk.ctypes.data, int(sizes[0, k]) // 8, got.ctypes.data, C.byref(nb), None) == 0, L.ulcx_last_error()
            assert consumed(nb.value, sizes[0, k])
        assert np.array_equal(got, seq[k]), k
    d.close()

    # ---- the ladder's slots and sizes: ladders of 1, 3 and 2 rungs on one encoder; every rung is what a plain call at that
    # setting writes on a freshly reset encoder
    plain = {}
    ref = u.BatchEncoder(B, CH, BS, RATE, MAXK)
    for setting in [(0, 50.0), (0, 30.0), (1, 64.0), (0, 70.0), (1, 96.0)]:
        ref.reset()
        plain[setting] = ref.encode(pcm[:, :K * BS], *setting)
    ref.close()
    enc = u.BatchEncoder(B, CH, BS, RATE, MAXK)
    for ladder in ([(0, 50.0)], [(0, 30.0), (1, 64.0), (0, 70.0)], [(1, 96.0), (0, 50.0)]):
        enc.reset()
        out, bits, wc, cplx = enc.encode_ladder(pcm[:, :K * BS], ladder)
        assert out.shape[0] == len(ladder) and enc.last_rungs() == len(ladder)
        for r, setting in enumerate(ladder):
            same_encoding((out[r], bits[r], wc, cplx), plain[setting])
    enc.close()
    assert not np.array_equal(plain[(0, 30.0)][1], plain[(0, 70.0)][1])


def test_payload_replaced(blocks):
    u = amd()
    L = u.lib()
    K = MAXK
    pays = {q: pack([(blocks[q][0][s, :K], blocks[q][1][s, :K]) for s in range(B)]) for q in (50.0, 20.0)}
    ref = u.BatchDecoder(B, CH, BS, MAXK)
    want_pcm, want_bits = ref.decode_packed(*pays[20.0], K)
    ref.close()
    assert consumed(want_bits, blocks[20.0][1][:, :K])
    d = u.BatchDecoder(B, CH, BS, MAXK)
    d.upload_payload(*pays[50.0])
    assert (d.index_resident(K) == K).all()
    d.upload_payload(*pays[20.0])
    first, n = np.array([1, 0, 2], np.int32), 2
    hp, hb = np.zeros((B, n * BS, CH), np.float32), np.zeros((B, n), np.int32)
    msg = refused(L.ulcx_decode_resident_range_host(d.h, p(first, C.c_int32), n, p(hp, C.c_float), p(hb, C.c_int32)), "ulcx_decode_resident_range_host")
    assert "not indexed" in msg
    assert (d.index_resident(K) == K).all()
    got_pcm, got_bits = d.decode_resident_range(first, n)
    for s in range(B):
        f = int(first[s])
        assert np.array_equal(got_bits[s], want_bits[s, f:f + n]), s
        assert np.array_equal(got_pcm[s], want_pcm[s, f * BS:(f + n) * BS]), s
    assert np.abs(got_pcm).max() > 0.01
    d.close()
