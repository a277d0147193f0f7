"""Index while encoding on the GPU (include/ulc_amd.h section 3: ulcx_index_begin_dev / ulcx_index_slots_* and
ulcx_decoder_set_resident_index): the index grown from slot-form buffers against the oracle's walk of the same blocks packed
(tests/seek_testlib.py: oracle_walk), entry for entry - offsets, generator states, counts and the {-1, 0} tail - and against
this library's own packed index.  The expected values are always the oracle's."""
import ctypes as C
import functools
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_testlib import amd as _amd, dev as _dev, to_dev as _t
import guarded_buffers as gb
from ulc_testlib import oracle, ptr, f32p, i32p, u8p, synth_pcm, same_bits
from seek_testlib import RATE, SEED0, geometries, pack, oracle_walk, oracle_pcm, damaged, expected_range

pytestmark = pytest.mark.gpu
GEOMS = sorted(geometries().keys())
A_WORD, A_BYTE = 4, 1                                       # the alignments of include/ulc_amd.h, "Caller buffers"


def _bytes8(bits):
    """d_bits as the encoder writes them: whole bytes."""
    return ((np.asarray(bits, np.int64) + 7) // 8 * 8).astype(np.int32)


def _walk(blocks, bits, ch, bs):
    """The oracle's walk of the blocks packed -> (byte offsets [K + 1], generator states [K + 1]); every block is walked."""
    host, nb = pack([(blocks, bits)])
    wbits, offs, seeds, inside = oracle_walk(host[0], int(nb[0]), ch, bs, len(bits))
    assert len(wbits) == len(bits) and inside and np.array_equal((wbits + 7) // 8, (np.asarray(bits) + 7) // 8)     # (the encoder's sizes are whole bytes)
    return offs, seeds


def _row(stride, offs, seeds, n=None):
    """A row of `stride` entries whose first n + 1 are the walk's, the rest {-1, 0}."""
    amd = _amd()
    n = len(offs) - 1 if n is None else n
    row = amd.new_index(1, stride)[0]
    row["ByteOffs"][:n + 1] = offs[:n + 1]
    row["RngState"][:n + 1] = seeds[:n + 1]
    return row


class DevIndex:
    """An index of R rows kept on the device and grown by ulcx_index_slots_dev calls."""

    def __init__(self, dec, R, stride):
        import torch
        self.dec, self.R, self.stride = dec, R, stride
        self.idx = torch.full((R, stride, 2), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        self.cnt = torch.full((R,), 0x5A5A5A5A, dtype=torch.int32, device=_dev())
        dec.index_begin_dev(R, self.idx.data_ptr(), stride, self.cnt.data_ptr())

    def append(self, blocks, bits):
        """blocks uint8 [R][K][slot], bits int32 [R][K]"""
        R, K, slot = blocks.shape
        assert R == self.R and bits.shape == (R, K)
        d_slots, d_bits = _t(blocks), _t(bits.astype(np.int32))
        self.dec.index_slots_dev(R, d_slots.data_ptr(), slot, d_bits.data_ptr(), K, self.idx.data_ptr(), self.stride, self.cnt.data_ptr())

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        amd = _amd()
        return self.idx.cpu().numpy().view(amd.INDEX_DTYPE).reshape(self.R, self.stride), self.cnt.cpu().numpy()


def _feed(dec, rows, stride, schedule):
    """rows: [(blocks [K][slot], bits8 [K])]; schedule: per call (blocks in the call's buffer, [blocks row r takes]).  A row that
    takes fewer than the call holds has d_bits 0 behind them (its slots still hold the stream's next blocks)."""
    R, slot = len(rows), rows[0][0].shape[1]
    di = DevIndex(dec, R, stride)
    pos = [0] * R
    for Kc, takes in schedule:
        blocks = np.zeros((R, Kc, slot), np.uint8)
        bits = np.zeros((R, Kc), np.int32)
        for r, (blk, b8) in enumerate(rows):
            have = min(Kc, len(b8) - pos[r])
            blocks[r, :have] = blk[pos[r]:pos[r] + have]
            bits[r, :takes[r]] = b8[pos[r]:pos[r] + takes[r]]
            pos[r] += takes[r]
        di.append(blocks, bits)
    return di.fetch(), pos


# ---------------------------------------------------------------------------------------------------------------------
# 1. the whole index of every geometry's streams, one call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_one_call_gives_the_oracles_walk_and_the_packed_index(geom):
    amd = _amd()
    bs, ch = geom
    streams = geometries()[geom]
    R, K = len(streams), max(len(bits) for _, _, bits, _ in streams)
    slot = streams[0][1].shape[1]
    blocks = np.zeros((R, K, slot), np.uint8)
    bits8 = np.zeros((R, K), np.int32)
    for r, (_, blk, bits, _) in enumerate(streams):
        blocks[r, :len(bits)] = blk
        bits8[r, :len(bits)] = _bytes8(bits)
    dec = amd.BatchDecoder(1, ch, bs, 2)                    # one stream, two blocks per call: neither limits the index
    index, count = dec.index_slots(blocks, bits8, index_stride=K + 3)
    dec.close()
    host, nbytes = pack([(blk, bits) for _, blk, bits, _ in streams])
    dec = amd.BatchDecoder(R, ch, bs, 2)
    pidx, pcnt = dec.index_packed(host, nbytes, K + 2)
    dec.close()
    for r, (name, blk, bits, _) in enumerate(streams):
        offs, seeds = _walk(blk, bits, ch, bs)
        assert count[r] == len(bits), (name, count[r])
        assert np.array_equal(index[r], _row(K + 3, offs, seeds)), f"{name}: differs from the oracle's walk"
    assert np.array_equal(count, pcnt) and np.array_equal(index, pidx), "differs from ulcx_index_packed_host of the packed blocks"


# ---------------------------------------------------------------------------------------------------------------------
# 2. chunk edges and appending
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiled(geom, L, rot):
    """The geometry's first stream (512 x 1: the hand-assembled one, 2048 x 2: the oracle-encoded one) tiled to L blocks from
    block `rot` on - blocks parse independently, so that is a valid stream - with the oracle's walk of it."""
    bs, ch = geom
    _, blk, bits, _ = geometries()[geom][0]
    pick = (np.arange(L) + rot) % len(bits)
    tb, tbits = np.ascontiguousarray(blk[pick]), bits[pick]
    offs, seeds = _walk(tb, tbits, ch, bs)
    return tb, _bytes8(tbits), offs, seeds


@pytest.mark.parametrize("geom,L,calls,R", [((512, 1), 130, (1, 63, 64, 2), 1), ((512, 1), 130, (1, 63, 64, 2), 3),
                                            ((512, 1), 130, (1, 63, 64, 2), 67), ((2048, 2), 160, (1, 63, 64, 32), 3)])
def test_chunk_edges_and_appending_give_one_index(geom, L, calls, R):
    amd = _amd()
    bs, ch = geom
    assert (geometries()[geom][0][3] is not None) == (geom == (2048, 2))
    rows, want = [], []
    for r in range(R):
        tb, b8, offs, seeds = _tiled(geom, L, 7 * (r % 4))  # four different rows, repeated
        rows.append((tb, b8))
        want.append(_row(L + 1, offs, seeds))
    want = np.stack(want)
    assert sum(calls) == L
    dec = amd.BatchDecoder(1, ch, bs, 2)
    (one, c1), _ = _feed(dec, rows, L + 1, [(L, [L] * R)])
    (app, c2), _ = _feed(dec, rows, L + 1, [(k, [k] * R) for k in calls])
    # rows that start each call from different counts: the first call gives row r 1 + r % 3 blocks, and row 0 is appended
    # to in every second call only
    sched, pos, call = [], [0] * R, 0
    while min(pos) < L:
        Kc = 3 if call == 0 else 40
        takes = [min(1 + r % 3 if call == 0 else Kc, L - pos[r]) for r in range(R)]
        if call % 2 == 1:
            takes[0] = 0
        pos = [p + t for p, t in zip(pos, takes)]
        sched.append((Kc, takes))
        call += 1
    (mix, c3), _ = _feed(dec, rows, L + 1, sched)
    dec.close()
    for what, idx, cnt in (("one call", one, c1), (f"calls of {calls}", app, c2), ("rows from different counts", mix, c3)):
        assert (cnt == L).all(), (what, cnt)
        bad = sorted(set(np.argwhere(idx != want)[:, 0].tolist()))
        assert not bad, f"{what}: rows {bad[:8]} differ from the oracle's walk"


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows of unequal length
# ---------------------------------------------------------------------------------------------------------------------
def test_rows_of_unequal_length_stop_where_their_sizes_end_and_grow_from_there():
    amd = _amd()
    geom, L, K1 = (2048, 2), 20, 9
    bs, ch = geom
    _, blk, bits, _ = geometries()[geom][0]
    blk, bits = blk[:L], bits[:L]
    offs, seeds = _walk(blk, bits, ch, bs)
    rows = [(blk, _bytes8(bits))] * 3
    ends = [5, 0, K1]                                       # d_bits 0 from block 5 / from block 0 / never
    dec = amd.BatchDecoder(1, ch, bs, 2)
    (idx, cnt), pos = _feed(dec, rows, L + 1, [(K1, ends)])
    assert list(cnt) == ends
    for r, n in enumerate(ends):
        assert np.array_equal(idx[r], _row(L + 1, offs, seeds, n)), f"row {r}: {n} blocks, then {{-1, 0}}"
    (idx, cnt), _ = _feed(dec, rows, L + 1, [(K1, ends), (L, [L - e for e in ends])])
    dec.close()
    assert (cnt == L).all()
    for r in range(3):
        assert np.array_equal(idx[r], _row(L + 1, offs, seeds)), f"row {r}: the second call appends behind block {ends[r]}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. wrong sizes and damaged blocks
# ---------------------------------------------------------------------------------------------------------------------
def _slots_walk(blocks, bits8, ch, bs):
    """The oracle, slot by slot: a row closes at the first block whose size is not positive or for which the oracle, decoding
    that slot on its own, reports 0 bits or a byte count other than d_bits / 8.  -> (offsets, generator states) of the n + 1
    entries."""
    lib = oracle()
    lib.orc_decode_stream_seeded.argtypes = [C.c_int, C.c_int, u8p, C.c_int, C.c_int, f32p, i32p, C.POINTER(C.c_uint32)]
    slot = blocks.shape[1]
    pcm = np.zeros((bs, ch), np.float32)
    b = np.zeros(1, np.int32)
    offs, seeds, sd = [0], [SEED0], C.c_uint32(SEED0)
    for k in range(len(bits8)):
        if bits8[k] <= 0 or bits8[k] // 8 > slot:
            break
        row = np.ascontiguousarray(blocks[k])
        b[0] = 0
        lib.orc_decode_stream_seeded(ch, bs, ptr(row, u8p), slot, 1, ptr(pcm, f32p), ptr(b, i32p), C.byref(sd))
        if b[0] == 0 or (int(b[0]) + 7) // 8 != int(bits8[k]) // 8:
            break
        offs.append(offs[-1] + int(bits8[k]) // 8)
        seeds.append(sd.value)
    return np.array(offs, np.int64), np.array(seeds, np.uint32)


# (block, seed of seek_testlib.damaged applied to that slot's bytes).  Found on the CPU with the oracle alone (seeds 0 .. 39 per
# block: two to six of them close the row at the damaged block): six that close the row there, one that changes a noise code
# and with it every later generator state, one that changes a coefficient's value only.
DAMAGE = [(2, 1), (5, 5), (7, 8), (9, 9), (3, 27), (6, 6), (4, 1), (8, 0)]
SIZES = [("plus", 0), ("plus", 6), ("plus", 11), ("minus", 0), ("minus", 4), ("minus", 11)]


def _damaged_rows():
    geom, L = (2048, 2), 12
    bs, ch = geom
    _, blk, bits, _ = geometries()[geom][0]
    blk, b8 = blk[:L], _bytes8(bits[:L])
    rows = [("clean", blk, b8)]
    for kind, k in SIZES:
        b = b8.copy()
        b[k] += 8 if kind == "plus" else -8
        rows.append((f"size of block {k} one byte {kind}", blk, b))
    for k, seed in DAMAGE:
        d = blk.copy()
        nb = int(b8[k]) // 8
        d[k, :nb] = damaged(blk[k, :nb], nb, seed)
        rows.append((f"block {k} damaged (seed {seed})", d, b8))
    return geom, L, rows


def test_wrong_sizes_and_damaged_blocks_close_the_row_where_the_oracle_stops():
    amd = _amd()
    geom, L, rows = _damaged_rows()
    bs, ch = geom
    walks = [_slots_walk(blk, b8, ch, bs) for _, blk, b8 in rows]
    stops = [len(o) - 1 for o, _ in walks]
    assert stops[0] == L
    assert stops[1:1 + len(SIZES)] == [k for _, k in SIZES], stops             # a wrong size closes the row at its block
    inside = sum(0 < n < L for n in stops[1 + len(SIZES):])
    print(f"damaged rows stop at {stops[1 + len(SIZES):]}: {inside} of {len(DAMAGE)} strictly inside the row")
    assert 2 * inside >= len(DAMAGE), stops
    dec = amd.BatchDecoder(1, ch, bs, 2)
    index, count = dec.index_slots(np.stack([blk for _, blk, _ in rows]), np.stack([b8 for _, _, b8 in rows]), index_stride=L + 1)
    dec.close()
    for r, (name, _, _) in enumerate(rows):
        offs, seeds = walks[r]
        assert count[r] == stops[r], f"{name}: {count[r]} blocks, the oracle stops at {stops[r]}"
        assert np.array_equal(index[r], _row(L + 1, offs, seeds)), name


# ---------------------------------------------------------------------------------------------------------------------
# 5 + 6. capacity, rows out of range, and the buffer contract
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_untouched_rows_and_the_buffer_contract():
    """Poisoned buffers between guards.  Row 0 has room for all of the call's blocks and more: the entries behind n0 + nBlocks
    keep the poison.  Rows 1 and 2 run out of entries (from 0 and from 3 blocks): the count is indexStride - 1 and the next
    row's entry 0 is not touched.  Rows 3 and 4 count -1 and indexStride blocks: left as they are.  Row 5 is shorter than the
    call.  The call runs on a stream of its own with a copy of the index enqueued right behind it."""
    import torch
    amd = _amd()
    geom, K, stride = (2048, 2), 10, 8
    bs, ch = geom
    _, blk, bits, _ = geometries()[geom][0]
    offs, seeds = _walk(blk[:20], bits[:20], ch, bs)
    b8 = _bytes8(bits)
    slot = blk.shape[1]
    R = 6
    wide = 16                                               # row 0 lives in a table of its own with room to spare
    n0 = [2, 0, 3, -1, stride, 1]
    first = [2, 0, 3, 0, 0, 1]                              # the stream's block in the call's slot 0
    blocks = np.stack([blk[f:f + K] for f in first])
    dbits = np.stack([b8[f:f + K] for f in first])
    dbits[5, 4:] = 0
    for tag, rows, st in (("wide", [0], wide), ("tight", [1, 2, 3, 4, 5], stride)):
        n = len(rows)
        a = gb.build(_dev(), [dict(name="d_slots", nbytes=n * K * slot, align=A_BYTE, role="in", guard=n * K * slot, row=slot, rows_per_stream=K),
                              dict(name="d_bits", nbytes=4 * n * K, align=A_WORD, role="in", guard=4 * n * K, row=4, rows_per_stream=K),
                              dict(name="d_index", nbytes=8 * n * st, align=A_WORD, role="inout", guard=8 * n * st, row=8, rows_per_stream=st),
                              dict(name="d_nBlocks", nbytes=4 * n, align=A_WORD, role="inout", guard=4096, row=4)])
        a.load("d_slots", blocks[rows]); a.load("d_bits", dbits[rows])
        before = a.fetch("d_index", amd.INDEX_DTYPE).reshape(n, st).copy()         # poison ...
        for i, r in enumerate(rows):
            if 0 <= n0[r] < st:
                before[i, :n0[r] + 1] = _row(st, offs, seeds, n0[r])[:n0[r] + 1]   # ... behind the entries the row has so far
        a.load("d_index", before); a.load("d_nBlocks", np.array([n0[r] for r in rows], np.int32))
        stream = torch.cuda.Stream(device=_dev())
        stream.wait_stream(torch.cuda.current_stream())                            # (the loads above)
        dec = amd.BatchDecoder(1, ch, bs, 2)
        with torch.cuda.stream(stream):
            dec.index_slots_dev(n, a.ptr("d_slots"), slot, a.ptr("d_bits"), K, a.ptr("d_index"), st, a.ptr("d_nBlocks"), stream=stream.cuda_stream)
            behind = a.view("d_index").clone()                                  # enqueued behind the call, no synchronisation
        torch.cuda.synchronize()
        dec.close()
        a.check()                                                                  # guards, and the two inputs unchanged
        got = a.fetch("d_index", amd.INDEX_DTYPE).reshape(n, st)
        cnt = a.fetch("d_nBlocks", np.int32)
        assert np.array_equal(behind.cpu().numpy().view(amd.INDEX_DTYPE).reshape(n, st), got), f"{tag}: a copy on the call's stream saw another index"
        for i, r in enumerate(rows):
            want = before[i].copy()
            if 0 <= n0[r] < st:
                m = min(K if r != 5 else 4, st - 1 - n0[r])
                last = min(n0[r] + K, st - 1)
                want[:n0[r] + m + 1] = _row(st, offs, seeds, n0[r] + m)[:n0[r] + m + 1]
                want["ByteOffs"][n0[r] + m + 1:last + 1] = -1
                want["RngState"][n0[r] + m + 1:last + 1] = 0
                assert cnt[i] == n0[r] + m, f"{tag} row {r}: count {cnt[i]}, expected {n0[r] + m}"
            else:
                assert cnt[i] == n0[r], f"{tag} row {r}: a count out of range was rewritten to {cnt[i]}"
            assert np.array_equal(got[i], want), f"{tag} row {r} (n0 {n0[r]}): entries other than n0+1 .. min(n0+nBlocks, stride-1) changed, or those are wrong"
        if tag == "tight":
            assert cnt[0] == stride - 1 and cnt[1] == stride - 1


def test_begin_opens_every_row_and_misaligned_pointers_are_refused():
    import torch
    amd = _amd()
    dec = amd.BatchDecoder(1, 2, 2048, 2)
    R, st = 5, 7
    a = gb.build(_dev(), [dict(name="d_index", nbytes=8 * R * st, align=A_WORD, role="out", guard=8 * R * st, row=8, rows_per_stream=st),
                          dict(name="d_nBlocks", nbytes=4 * R, align=A_WORD, role="out", guard=4096, row=4)])
    dec.index_begin_dev(R, a.ptr("d_index"), st, a.ptr("d_nBlocks"))
    torch.cuda.synchronize()
    a.check()
    assert np.array_equal(a.fetch("d_index", amd.INDEX_DTYPE).reshape(R, st), amd.new_index(R, st))
    assert (a.fetch("d_nBlocks", np.int32) == 0).all()
    for name in ("d_index", "d_nBlocks"):
        args = dict(d_index=a.ptr("d_index"), d_nBlocks=a.ptr("d_nBlocks"))
        args[name] += 2
        with pytest.raises(amd.UlcError, match="not aligned"):
            dec.index_begin_dev(R, args["d_index"], st, args["d_nBlocks"])
    torch.cuda.synchronize()
    a.check()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7 + 8. from the encoder, into range calls and the resident decoder
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _encoded():
    """3 streams x 2 calls x 6 blocks through a two-rung ladder call (VBR 50 / CBR 64), every call's 2 x 3 rows indexed right
    behind it on the same stream -> what the device left: the blocks, their sizes, the index grown call by call, the packed
    payloads and ulcx_index_packed_dev's index of them."""
    import torch
    amd = _amd()
    bs, ch, B, K, CALLS, RUNGS = 2048, 2, 3, 6, 2, 2
    R, L = RUNGS * B, CALLS * K
    pcm = np.stack([synth_pcm(s, L * bs, ch, RATE, transient=True, seed=21) for s in range(B)]).reshape(B, L, bs, ch)
    enc = amd.BatchEncoder(B, ch, bs, RATE, K)
    dec = amd.BatchDecoder(R, ch, bs, K)
    slot, stride = enc.slot, L + 1
    dev = _dev()
    allb = torch.zeros((R, L, slot), dtype=torch.uint8, device=dev)
    allbits = torch.zeros((R, L), dtype=torch.int32, device=dev)
    di = DevIndex(dec, R, stride)
    for c in range(CALLS):
        d_pcm = _t(pcm[:, c * K:(c + 1) * K])
        out = torch.zeros((RUNGS, B, K, slot), dtype=torch.uint8, device=dev)
        bits = torch.zeros((RUNGS, B, K), dtype=torch.int32, device=dev)
        enc.encode_dev_ladder([(amd.MODE_VBR, 50.0, 0.0), (amd.MODE_CBR, 64.0, 0.0)], d_pcm.data_ptr(), K, out.data_ptr(), bits.data_ptr())
        dec.index_slots_dev(R, out.data_ptr(), slot, bits.data_ptr(), K, di.idx.data_ptr(), stride, di.cnt.data_ptr())
        allb[:, c * K:(c + 1) * K] = out.view(R, K, slot)
        allbits[:, c * K:(c + 1) * K] = bits.view(R, K)
    pstride = L * slot
    pay = torch.zeros((R, pstride), dtype=torch.uint8, device=dev)
    pbytes = torch.zeros((R,), dtype=torch.int32, device=dev)
    rc = amd.lib().ulcx_pack_streams_dev(0, R, L, slot, allb.data_ptr(), allbits.data_ptr(), pay.data_ptr(), pstride, pbytes.data_ptr(), None, None)
    assert rc == 0
    pidx = torch.zeros((R, stride, 2), dtype=torch.int32, device=dev)
    pcnt = torch.zeros((R,), dtype=torch.int32, device=dev)
    dec.index_packed_dev(pay.data_ptr(), pstride, pbytes.data_ptr(), L, pidx.data_ptr(), pcnt.data_ptr())
    index, count = di.fetch()
    # blocks 4 .. 8 of every row with the grown index
    first, N = 4, 5
    d_first = _t(np.full(R, first, np.int32))
    d_out = torch.zeros((R, N, bs, ch), dtype=torch.float32, device=dev)
    d_ob = torch.zeros((R, N), dtype=torch.int32, device=dev)
    dec.decode_range_dev(pay.data_ptr(), pstride, pbytes.data_ptr(), di.idx.data_ptr(), stride, di.cnt.data_ptr(), d_first.data_ptr(), N,
                         d_out.data_ptr(), d_ob.data_ptr())
    torch.cuda.synchronize()
    r = dict(bs=bs, ch=ch, R=R, L=L, slot=slot, blocks=allb.cpu().numpy(), bits=allbits.cpu().numpy(), index=index.copy(), count=count.copy(),
             pindex=pidx.cpu().numpy().view(amd.INDEX_DTYPE).reshape(R, stride), pcount=pcnt.cpu().numpy(),
             payload=pay.cpu().numpy(), pbytes=pbytes.cpu().numpy(), first=first, N=N, pcm=d_out.cpu().numpy(), obits=d_ob.cpu().numpy())
    enc.close(); dec.close()
    return r


def test_index_grown_behind_encode_calls_equals_the_packed_index_and_the_oracle():
    e = _encoded()
    assert (e["count"] == e["L"]).all() and np.array_equal(e["count"], e["pcount"])
    assert np.array_equal(e["index"], e["pindex"]), "differs from ulcx_index_packed_dev of the packed payload"
    for r in range(e["R"]):
        offs, seeds = _walk(e["blocks"][r], e["bits"][r], e["ch"], e["bs"])
        assert np.array_equal(e["index"][r], _row(e["L"] + 1, offs, seeds)), f"row {r}: differs from the oracle's walk"
        assert e["pbytes"][r] == offs[-1]


def test_range_decode_with_the_grown_index_is_the_oracles_slice():
    e = _encoded()
    for r in range(e["R"]):
        ref, rbits = oracle_pcm(e["blocks"][r], e["ch"], e["bs"])
        want, wb = expected_range(ref, rbits, e["first"], e["N"])
        assert np.array_equal(e["obits"][r], wb), (r, e["obits"][r], wb)
        assert same_bits(e["pcm"][r], want, shape=False), f"row {r}: blocks {e['first']} .. differ from the oracle's sequential decode"


def test_resident_decoder_takes_a_stored_index():
    amd = _amd()
    e = _encoded()
    R, N = e["R"], e["N"]
    first = np.array([4, 0, 7, 2, 5, 1], np.int32)
    dec = amd.BatchDecoder(R, e["ch"], e["bs"], N + 1)
    dec.upload_payload(e["payload"], e["pbytes"])
    with pytest.raises(amd.UlcError):
        dec.decode_resident_range(first, N)                 # no index yet
    dec.set_resident_index(e["index"], e["count"])
    p1, b1 = dec.decode_resident_range(first, N)
    # indexes that ulcx_index_check refuses: the decoder keeps the one it has
    bad = e["index"].copy(); bad["RngState"][2, 0] = 7
    late = e["index"].copy(); late["ByteOffs"][3, e["L"]] = e["pbytes"][3] + 1
    flat = e["index"].copy(); flat["ByteOffs"][1, 5] = flat["ByteOffs"][1, 4]
    for idx, cnt in ((bad, e["count"]), (late, e["count"]), (flat, e["count"]), (e["index"], np.full(R, e["L"] + 1, np.int32))):
        with pytest.raises(amd.UlcError, match="stream"):
            dec.set_resident_index(idx, cnt)
    p2, b2 = dec.decode_resident_range(first, N)
    assert np.array_equal(b1, b2) and same_bits(p1, p2, shape=False), "a refused index changed the decoder"
    dec.upload_payload(e["payload"], e["pbytes"])           # a new upload drops the index
    with pytest.raises(amd.UlcError):
        dec.decode_resident_range(first, N)
    assert np.array_equal(dec.index_resident(e["L"]), e["count"])
    p3, b3 = dec.decode_resident_range(first, N)
    dec.close()
    assert np.array_equal(b1, b3) and same_bits(p1, p3, shape=False), "stored index and ulcx_decoder_index_resident decode differently"
    for r in range(R):
        ref, rbits = oracle_pcm(e["blocks"][r], e["ch"], e["bs"])
        want, wb = expected_range(ref, rbits, int(first[r]), N)
        assert np.array_equal(b1[r], wb) and same_bits(p1[r], want, shape=False), f"row {r} from block {first[r]}"
