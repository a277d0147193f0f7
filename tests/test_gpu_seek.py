"""Block index and seek on the GPU (include/ulc_amd.h section 3): ulcx_index_packed_* against the oracle's block sizes and
generator states, ulcx_decode_range_* against slices of the oracle's sequential decode - bit patterns, the noise included -,
the state a range call leaves, the cut launches, PCM16 output and the front-end's -blocks: option.
The reference is always the oracle (tests/seek_testlib.py), never this library's own sequential decode."""
import ctypes as C
import os
import struct
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from gpu_testlib import amd as _amd
from seek_testlib import (RATE, SEED0, ORACLE_BLOCKS, geometries, oracle_stream, pack, oracle_seeds, oracle_pcm, expected_range,
                          switched_starts, damaged, oracle_walk)
from ulc_testlib import oracle_decode_stream, run_tool, same_bits

pytestmark = pytest.mark.gpu
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
MAXK = 4                                                    # maxBlocksPerCall of the small decoders: range calls of 3 blocks
GEOMS = sorted(geometries().keys())


def _group(geom):
    streams = geometries()[geom]
    host, nbytes = pack([(blocks, bits) for _, blocks, bits, _ in streams])
    return streams, host, nbytes


# ---------------------------------------------------------------------------------------------------------------------
# 1. the index against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_index_matches_the_oracle(geom):
    amd = _amd()
    bs, ch = geom
    streams, host, nbytes = _group(geom)
    L = amd.lib()
    dec = amd.BatchDecoder(len(streams), ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)      # 40 blocks in one call of a decoder of 4 blocks per call
    dec.close()
    assert index.shape == (len(streams), ORACLE_BLOCKS + 1) and index.dtype.itemsize == 8
    for s, (name, blocks, bits, _) in enumerate(streams):
        K = len(bits)
        seeds = oracle_seeds(blocks, ch, bs)
        changed = int((seeds[1:] != seeds[:-1]).sum())
        print(f"{name}: {K} blocks, {changed} change the generator state")
        assert changed * 10 >= K * 9, f"{name}: only {changed} of {K} blocks change the generator state - a wrong state could pass"
        assert count[s] == K, (name, count[s])
        offs = np.concatenate([[0], np.cumsum((bits.astype(np.int64) + 7) // 8)])
        assert np.array_equal(index["ByteOffs"][s, :K + 1], offs), name
        # the same by the host walk, one block at a time
        off, pay = 0, np.ascontiguousarray(host[s])
        for k in range(K):
            assert off == index["ByteOffs"][s, k], (name, k)
            off += L.ulcx_block_extent_bytes(pay.ctypes.data + off, ch, bs, int(nbytes[s]) - off)
        assert off == index["ByteOffs"][s, K] == nbytes[s], name
        assert np.array_equal(index["RngState"][s, :K + 1], seeds), f"{name}: generator states differ from the oracle's"
        assert (index["ByteOffs"][s, K + 1:] == -1).all() and (index["RngState"][s, K + 1:] == 0).all(), f"{name}: unused entries"


# ---------------------------------------------------------------------------------------------------------------------
# 2. truncated and empty payloads
# ---------------------------------------------------------------------------------------------------------------------
def test_index_of_truncated_and_empty_payloads():
    amd = _amd()
    bs, ch = 2048, 2
    name, blocks, bits, _ = geometries()[(bs, ch)][0]
    K = len(bits)
    host1, nb1 = pack([(blocks, bits)])
    host = np.repeat(host1, 5, axis=0)
    offs = np.concatenate([[0], np.cumsum((bits.astype(np.int64) + 7) // 8)])
    cut = np.array([nb1[0], offs[17] + (offs[18] - offs[17]) // 2, offs[9], 0, offs[30] + 1], np.int32)
    want = [K, 17, 9, 0, 30]
    seeds = oracle_seeds(blocks, ch, bs)
    dec = amd.BatchDecoder(5, ch, bs, MAXK)
    index, count = dec.index_packed(host, cut, ORACLE_BLOCKS)
    dec.close()
    assert list(count) == want, list(count)
    for s, n in enumerate(want):
        assert np.array_equal(index["ByteOffs"][s, :n + 1], offs[:n + 1]), s          # the entries in front of the cut are unchanged
        assert np.array_equal(index["RngState"][s, :n + 1], seeds[:n + 1]), s
        assert (index["ByteOffs"][s, n + 1:] == -1).all() and (index["RngState"][s, n + 1:] == 0).all(), s
    assert index["ByteOffs"][3, 0] == 0 and index["RngState"][3, 0] == SEED0


# ---------------------------------------------------------------------------------------------------------------------
# 2b. damaged payloads: the index and the decoder agree with the oracle, and so with each other
# ---------------------------------------------------------------------------------------------------------------------
# Seeds of seek_testlib.damaged(), found on the CPU with the oracle alone (of 6000 seeds per stream about one in 300 changes a
# block's size and still lets the oracle run all 40 blocks, one in 10 stops it; most overwrite a coefficient's value).  Per
# stream: six that change a size without stopping the walk, six that stop it, four that change no size.
DAMAGE_SEEDS = {
    (2048, 2): [92, 1734, 2871, 3651, 4324, 4554, 14, 77, 80, 102, 123, 315, 0, 1, 2, 3],
    (4096, 2): [467, 938, 955, 1806, 3272, 3750, 35, 43, 47, 52, 94, 343, 0, 1, 2, 3],
}


@pytest.mark.parametrize("geom", sorted(DAMAGE_SEEDS))
def test_index_and_decode_of_damaged_payloads_match_the_oracle(geom):
    """Sixteen copies of one payload, each with one nybble overwritten inside its first half.  The index (count, offsets,
    generator states) and the bits a packed decode reports must be what the oracle's decoder gives when it walks the same
    bytes block by block (seek_testlib.oracle_walk): one walk serves both calls, and a range call trusts the index.  The
    samples of the packed decode are the oracle's too, bit for bit, up to the block where the walk stops, and zero behind it."""
    amd = _amd()
    bs, ch = geom
    K, seeds = ORACLE_BLOCKS, DAMAGE_SEEDS[geom]
    oracle_coded = {g: int((np.asarray(st[0][3]) != 0x10).sum()) for g, st in geometries().items() if st[0][3] is not None}
    assert geom == (2048, 2) or oracle_coded[geom] == max(oracle_coded.values()), f"{geom} is not the most window-switched stream: {oracle_coded}"
    name, blocks, bits, _ = geometries()[geom][0]
    host1, nb1 = pack([(blocks, bits)])
    nbytes = int(nb1[0])
    host = np.stack([damaged(host1[0], nbytes, sd) for sd in seeds])
    nb = np.full(len(seeds), nbytes, np.int32)
    clean = oracle_walk(host1[0], nbytes, ch, bs, K)
    assert len(clean[0]) == K and clean[3]
    walks = [oracle_walk(host[s], nbytes, ch, bs, K) for s in range(len(seeds))]
    # the inputs stress the walk: enough damages end it early, enough change a block's size and let it go on to the last block;
    # and no expected value comes from the zeros behind a payload
    stopped = sum(len(w[0]) < K for w in walks)
    resized = sum(len(w[0]) == K and not np.array_equal(w[0], clean[0]) for w in walks)
    print(f"{name}: {stopped} of {len(seeds)} damages stop the oracle before block {K}, {resized} change a block's size and run all {K}")
    assert stopped >= 4 and resized >= 4, (stopped, resized)
    assert all(w[3] for w in walks), "a walked block ends behind its payload"
    dec = amd.BatchDecoder(len(seeds), ch, bs, K)
    index, count = dec.index_packed(host, nb, K)
    dec.close()
    dec = amd.BatchDecoder(len(seeds), ch, bs, K)
    gpcm, gbits = dec.decode_packed(host, nb, K)
    dec.close()
    for s, (wbits, woffs, wseeds, _) in enumerate(walks):
        n = len(wbits)
        what = f"{name}, damage {seeds[s]} ({n} blocks)"
        assert count[s] == n, f"{what}: the index counts {count[s]}"
        assert np.array_equal(index["ByteOffs"][s, :n + 1], woffs), what
        assert np.array_equal(index["RngState"][s, :n + 1], wseeds), f"{what}: generator states differ from the oracle's"
        assert (index["ByteOffs"][s, n + 1:] == -1).all() and (index["RngState"][s, n + 1:] == 0).all(), f"{what}: unused entries"
        want = np.zeros(K, np.int32)
        want[:n] = wbits
        assert np.array_equal(gbits[s], want), f"{what}: the decode reports {gbits[s]}, the oracle {want}"
        # the samples: the damaged payload cut into slot rows at the walk's offsets, decoded by the oracle in one run
        rows = np.zeros((max(n, 1), 2 * ch * bs + 16), np.uint8)
        for k in range(n):
            rows[k, :woffs[k + 1] - woffs[k]] = host[s, woffs[k]:woffs[k + 1]]
        rc, rpcm, rbits = oracle_decode_stream(rows[:n], ch, bs) if n else (0, np.zeros((0, ch), np.float32), wbits)
        assert rc == 0 and np.array_equal(rbits, wbits), what
        assert same_bits(gpcm[s][:n * bs], rpcm, shape=False), f"{what}: the decoded samples differ from the oracle's"
        assert not gpcm[s][n * bs:].any(), f"{what}: samples behind block {n}, where the walk stops"


# ---------------------------------------------------------------------------------------------------------------------
# 3. a range equals the slice of the sequential decode
# ---------------------------------------------------------------------------------------------------------------------
def _starts(K, wc):
    st = [0, 1, K - 1]
    if wc is not None:
        sw = switched_starts(wc)
        assert len(sw) >= 3, f"only {len(sw)} starts behind a window-switched block"
        st += sw
    else:
        st += [5, 12]
    return st + [K - 2, K]                                   # running past the stream's end; starting at it


@pytest.mark.parametrize("geom", GEOMS)
def test_range_equals_the_slice_of_the_oracles_decode(geom):
    amd = _amd()
    bs, ch = geom
    streams, host, nbytes = _group(geom)
    B, N = len(streams), MAXK - 1
    refs = [oracle_pcm(blocks, ch, bs) for _, blocks, _, _ in streams]
    starts = [_starts(len(bits), wc) for _, _, bits, wc in streams]
    dec = amd.BatchDecoder(B, ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    dec.upload_payload(host, nbytes)
    assert np.array_equal(dec.index_resident(ORACLE_BLOCKS), count)
    with pytest.raises(amd.UlcError):
        dec.decode_range(host, nbytes, index, count, np.zeros(B, np.int32), MAXK)          # one row is the block in front
    with pytest.raises(amd.UlcError):
        dec.decode_range(host, nbytes, index, count, np.full(B, -1, np.int32), N)          # refused by the host form
    checked = 0
    for i in range(max(len(st) for st in starts)):
        # the streams of one call start at different blocks (the second stream walks its list from the other end)
        first = np.array([st[(i if s % 2 == 0 else -1 - i) % len(st)] for s, st in enumerate(starts)], np.int32)
        pcm, gb = dec.decode_range(host, nbytes, index, count, first, N)
        pcm2, gb2 = dec.decode_resident_range(first, N)
        for s, (name, _, _, _) in enumerate(streams):
            want, wb = expected_range(refs[s][0], refs[s][1], int(first[s]), N)
            assert np.array_equal(gb[s], wb), f"{name}: bits of blocks {first[s]}.. are {gb[s]}, the oracle's {wb}"
            got = pcm[s].reshape(N, bs, ch)
            for k in range(N):
                assert same_bits(got[k], want[k], shape=False), f"{name}: block {first[s] + k} (range from {first[s]}) differs from the oracle's sequential decode"
            assert np.array_equal(gb2[s], wb) and same_bits(pcm2[s], want, shape=False), f"{name}: resident form, range from {first[s]}"
            checked += 1
    dec.close()
    assert checked >= 7 * B


def test_a_start_outside_the_index_gives_a_stream_of_zero_bits():
    """Device form: d_first outside [0, d_indexBlocks] cannot be refused without a synchronisation - that stream reports 0
    bits and silence, its neighbours are decoded."""
    import torch
    amd = _amd()
    bs, ch = 2048, 2
    streams, host, nbytes = _group((bs, ch))
    B, N = len(streams), MAXK - 1
    dev = torch.device("cuda", 0)
    dec = amd.BatchDecoder(B, ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pay, d_nb, d_idx, d_cnt = t(host), t(nbytes), t(index.view(np.int32).reshape(B, -1)), t(count)
    for bad in (-1, int(count[1]) + 1, 1 << 30):
        d_first = t(np.array([4, bad], np.int32))
        pcm = torch.full((B, N, bs, ch), 7.0, dtype=torch.float32, device=dev); bits = torch.full((B, N), 7, dtype=torch.int32, device=dev)
        dec.decode_range_dev(d_pay.data_ptr(), host.shape[1], d_nb.data_ptr(), d_idx.data_ptr(), index.shape[1], d_cnt.data_ptr(),
                             d_first.data_ptr(), N, pcm.data_ptr(), bits.data_ptr())
        torch.cuda.synchronize()
        assert (bits[1] == 0).all() and (pcm[1] == 0).all(), bad
        want, wb = expected_range(*oracle_pcm(streams[0][1], ch, bs), 4, N)
        assert np.array_equal(bits[0].cpu().numpy(), wb) and same_bits(pcm[0].cpu().numpy(), want, shape=False), bad
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the state a range call leaves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (4096, 2), (2048, 3)])
def test_state_after_a_range_call_is_the_sequential_decoders(geom):
    amd = _amd()
    bs, ch = geom
    streams, host, nbytes = _group(geom)
    B, N = len(streams), MAXK - 1
    refs = [oracle_pcm(blocks, ch, bs) for _, blocks, _, _ in streams]
    Ks = [len(bits) for _, _, bits, _ in streams]
    dec = amd.BatchDecoder(B, ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)

    def check(pcm, gb, first, n, what):
        for s, (name, _, _, _) in enumerate(streams):
            want, wb = expected_range(refs[s][0], refs[s][1], int(first[s]), n)
            assert np.array_equal(gb[s], wb), f"{what}: {name}: bits {gb[s]} vs the oracle's {wb}"
            assert same_bits(pcm[s], want, shape=False), f"{what}: {name}: blocks {first[s]}.. differ from the oracle's"

    # a packed call behind a range call continues with the next block (lapping, LastSubBlockSize, generator, read position)
    sw = switched_starts(streams[0][3])
    for f0 in (7, sw[0] - 1, sw[1]):                                         # (the range ends on / starts behind a window-switched block)
        first = np.array([f0] + [Ks[s] - 6 for s in range(1, B)], np.int32)
        check(*dec.decode_range(host, nbytes, index, count, first, N), first, N, f"range from {f0}")
        check(*dec.decode_packed(host, nbytes, MAXK), first + N, MAXK, f"packed call behind the range from {f0}")   # (the second stream ends inside it)
        if B > 1:
            assert dec.decode_packed(host, nbytes, 2)[1][1].tolist() == [0, 0], "a stream that ended stays ended"
    # backwards after forwards: as on a fresh decoder
    fwd = np.array([30] + [15] * (B - 1), np.int32)
    back = np.array([5] + [2] * (B - 1), np.int32)
    check(*dec.decode_range(host, nbytes, index, count, fwd, N), fwd, N, "forwards")
    p1, b1 = dec.decode_range(host, nbytes, index, count, back, N)
    check(p1, b1, back, N, "backwards")
    fresh = amd.BatchDecoder(B, ch, bs, MAXK)
    p2, b2 = fresh.decode_range(host, nbytes, index, count, back, N)
    fresh.close()
    assert np.array_equal(b1, b2) and same_bits(p1, p2, shape=False)
    check(*dec.decode_packed(host, nbytes, MAXK), back + N, MAXK, "packed call behind the backward range")
    dec.close()


def test_range_call_mixed_with_slot_calls_on_a_one_stream_decoder_keeps_the_chain():
    amd = _amd()
    bs, ch = 2048, 2
    name, blocks, bits, _ = geometries()[(bs, ch)][0]
    host, nbytes = pack([(blocks, bits)])
    ref, rbits = oracle_pcm(blocks, ch, bs)
    dec = amd.BatchDecoder(1, ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    N = MAXK - 1
    p, b = dec.decode(blocks[None, 0:3])
    assert np.array_equal(b[0], rbits[0:3]) and same_bits(p[0], ref[0:3], shape=False)
    p, b = dec.decode_range(host, nbytes, index, count, np.array([3], np.int32), N)
    assert np.array_equal(b[0], rbits[3:6]) and same_bits(p[0], ref[3:6], shape=False)
    p, b = dec.decode(blocks[None, 6:10])                                 # the slot form goes on where the range ended
    assert np.array_equal(b[0], rbits[6:10]) and same_bits(p[0], ref[6:10], shape=False)
    p, b = dec.decode_range(host, nbytes, index, count, np.array([20], np.int32), N)      # a jump, then slots again
    assert np.array_equal(b[0], rbits[20:23]) and same_bits(p[0], ref[20:23], shape=False)
    p, b = dec.decode(blocks[None, 23:27])
    assert np.array_equal(b[0], rbits[23:27]) and same_bits(p[0], ref[23:27], shape=False)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cuts
# ---------------------------------------------------------------------------------------------------------------------
def _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch, pcm16=False):
    import torch
    dev = torch.device("cuda", 0)
    B = host.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_pay, d_nb, d_idx, d_cnt, d_first = t(host), t(nbytes), t(index.view(np.int32).reshape(B, -1)), t(count), t(first)
    pcm = torch.zeros(B, N, bs, ch, dtype=torch.int16 if pcm16 else torch.float32, device=dev)
    bits = torch.zeros(B, N, dtype=torch.int32, device=dev)
    dec.decode_range_dev(d_pay.data_ptr(), host.shape[1], d_nb.data_ptr(), d_idx.data_ptr(), index.shape[1], d_cnt.data_ptr(),
                         d_first.data_ptr(), N, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm, bits


def test_few_long_streams_take_the_even_cut():
    """8 streams x 512 blocks from random starts: the synthesis is cut evenly over the device (ulcx_dec_split_plan), every
    workgroup entering its stream somewhere inside the range."""
    amd = _amd()
    bs, ch, B, N, L = 2048, 2, 8, 512, 600
    two = [oracle_stream(bs, ch, 50.0, sid, 11, L) for sid in (3, 4)]           # payloads repeated from two distinct streams
    host2, nb2 = pack([(blk, bits) for blk, bits, _ in two])
    host, nbytes = host2[np.arange(B) % 2], nb2[np.arange(B) % 2]
    refs = [oracle_pcm(blk, ch, bs) for blk, _, _ in two]
    first = np.random.default_rng(5).integers(0, L - N + 1, B).astype(np.int32)
    first[0], first[1] = 0, L - N
    dec = amd.BatchDecoder(B, ch, bs, N + 1)
    index, count = dec.index_packed(host, nbytes, L)
    assert (count == L).all()
    pcm, bits = _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch)
    grid, whole, resident = dec.last_cut()
    print(f"8 x 512: {grid} workgroups, {whole} whole streams, {resident} resident")
    for s in range(B):
        want, wb = expected_range(refs[s % 2][0], refs[s % 2][1], int(first[s]), N)
        assert np.array_equal(bits[s].cpu().numpy(), wb), s
        assert same_bits(pcm[s].cpu().numpy(), want, shape=False), f"stream {s} from block {first[s]}"
    # the state behind the cut launch: a packed call continues
    nxt, nb = dec.decode_packed(host, nbytes, 8)
    for s in range(B):
        want, wb = expected_range(refs[s % 2][0], refs[s % 2][1], int(first[s]) + N, 8)
        assert np.array_equal(nb[s], wb) and same_bits(nxt[s], want, shape=False), f"stream {s}: packed call behind the cut range"
    dec.close()
    assert resident > 0 and grid > 0 and whole == 0, f"expected an even cut, got {grid} workgroups / {whole} whole streams"


def test_many_short_streams_report_the_tail_cut():
    """1600 stereo streams x 7 blocks at BlockSize 2048: one whole round on an MI355X's 1536 resident workgroups and a last
    round of 64 streams, which a range call cuts into pieces of 2 blocks (ulcx_dec_range_tail_plan: in a range call a
    whole-stream workgroup runs the block in front of its range too, so short calls are worth cutting).  Eight streams -
    of the whole round, of the cut round, at their edge - are compared with the oracle, then the cut the call reports."""
    amd = _amd()
    bs, ch, B, N = 2048, 2, 1600, 7
    base = [oracle_stream(bs, ch, q, sid) for q, sid in ((50.0, 3), (50.0, 4), (35.0, 5), (65.0, 6))]
    host4, nb4 = pack([(blk, bits) for blk, bits, _ in base])
    pick = np.arange(B) % 4
    host, nbytes = host4[pick], nb4[pick]
    refs = [oracle_pcm(blk, ch, bs) for blk, _, _ in base]
    first = np.random.default_rng(9).integers(0, ORACLE_BLOCKS - N + 1, B).astype(np.int32)
    first[0], first[B - 1] = 0, ORACLE_BLOCKS - N
    dec = amd.BatchDecoder(B, ch, bs, N + 1)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    pcm, bits = _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch)
    grid, whole, resident = dec.last_cut()
    L = amd.lib()
    full = C.c_int32(0)
    tail = L.ulcx_dec_range_tail_plan(B, N, resident, C.byref(full))
    print(f"1600 x 7: {grid} workgroups, {whole} whole streams, {resident} resident; "
          f"split plan {L.ulcx_dec_split_plan(B, N, resident)}, range tail plan {tail} + {full.value}")
    for s in (0, 1, 2, 3, 777, resident - 1, resident % B, (resident + 1) % B, B - 2, B - 1):
        want, wb = expected_range(refs[s % 4][0], refs[s % 4][1], int(first[s]), N)
        assert np.array_equal(bits[s].cpu().numpy(), wb), s
        assert same_bits(pcm[s].cpu().numpy(), want, shape=False), f"stream {s} from block {first[s]}"
    nxt, nb = dec.decode_packed(host, nbytes, 4)             # the state behind the cut launch
    for s in (0, 3, resident - 1, resident % B, B - 2, B - 1):
        want, wb = expected_range(refs[s % 4][0], refs[s % 4][1], int(first[s]) + N, 4)
        assert np.array_equal(nb[s], wb) and same_bits(nxt[s], want, shape=False), f"stream {s}: packed call behind the cut range"
    dec.close()
    assert grid > 0 and whole > 0, f"expected the tail cut, got {grid} workgroups / {whole} whole streams ({resident} resident)"
    assert (grid, whole) == (full.value + tail, full.value), (grid, whole, tail, full.value)


def test_range_call_takes_the_cut_of_the_last_round():
    """A batch shaped for the tail plan whatever the device's residency (as tests/test_gpu_parity.py shapes its own): whole
    rounds + a last round two thirds full, 24 blocks.  The range call must report that cut, and streams of the whole rounds,
    of the cut round and at its edges must equal the oracle."""
    amd = _amd()
    bs, ch, N = 2048, 2, 24
    probe = amd.BatchDecoder(8, ch, bs, N + 1)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    B = resident + resident * 2 // 3
    L = amd.lib()
    full = C.c_int32(0)
    tail = L.ulcx_dec_tail_plan(B, N, resident, C.byref(full))
    assert L.ulcx_dec_split_plan(B, N, resident) == 0 and tail > 0 and full.value == resident, (B, resident, tail)
    base = [oracle_stream(bs, ch, q, sid) for q, sid in ((50.0, 3), (50.0, 4), (35.0, 5), (65.0, 6))]
    host4, nb4 = pack([(blk, bits) for blk, bits, _ in base])
    pick = np.arange(B) % 4
    host, nbytes = host4[pick], nb4[pick]
    refs = [oracle_pcm(blk, ch, bs) for blk, _, _ in base]
    first = np.random.default_rng(21).integers(0, ORACLE_BLOCKS - N + 1, B).astype(np.int32)
    first[0], first[resident] = 0, 0                         # (a range from block 0 in a whole-stream workgroup and in the cut round)
    first[B - 1] = ORACLE_BLOCKS - N + 5                     # the last stream runs past its end
    dec = amd.BatchDecoder(B, ch, bs, N + 1)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    pcm, bits = _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch)
    grid, whole, res2 = dec.last_cut()
    print(f"{B} x {N}: {grid} workgroups, {whole} whole streams, {res2} resident")
    assert whole == full.value and grid == full.value + tail, (grid, whole, tail)
    for s in (0, 1, resident - 1, resident, resident + 1, resident + (B - resident) // 2, B - 2, B - 1):
        want, wb = expected_range(refs[s % 4][0], refs[s % 4][1], int(first[s]), N)
        assert np.array_equal(bits[s].cpu().numpy(), wb), s
        assert same_bits(pcm[s].cpu().numpy(), want, shape=False), f"stream {s} from block {first[s]}"
    nxt, nb = dec.decode_packed(host, nbytes, 4)             # the state behind the cut launch
    for s in (0, resident, resident + 7, B - 1):
        want, wb = expected_range(refs[s % 4][0], refs[s % 4][1], int(first[s]) + N, 4)
        assert np.array_equal(nb[s], wb) and same_bits(nxt[s], want, shape=False), f"stream {s}: packed call behind the cut range"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. PCM16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (1024, 6)])
def test_pcm16_form_is_the_float_form_converted(geom):
    import torch
    amd = _amd()
    bs, ch = geom
    streams, host, nbytes = _group(geom)
    B, N = len(streams), MAXK - 1
    dec = amd.BatchDecoder(B, ch, bs, MAXK)
    index, count = dec.index_packed(host, nbytes, ORACLE_BLOCKS)
    for f in (0, 9, 21):
        first = np.full(B, f, np.int32)
        yf, bf = _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch)
        y16, b16 = _device_range(amd, dec, host, nbytes, index, count, first, N, bs, ch, pcm16=True)
        want = torch.clamp(torch.round(yf * 32768.0), -32768, 32767).to(torch.int16)          # lrintf(clamp(x * 2^15)), WavIO_Helper.c:56-63
        assert torch.equal(b16, bf) and torch.equal(y16, want), f"range from {f}"
        assert (bf > 0).any()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the front-end
# ---------------------------------------------------------------------------------------------------------------------
def _write_ulc(path, blocks, bits, bs, ch):
    sizes = (bits + 7) // 8
    payload = b"".join(blocks[k, :sizes[k]].tobytes() for k in range(len(bits)))
    kbps = int(np.rint(len(payload) * 8.0 * RATE / 1000.0 / (bs * len(bits))))
    with open(path, "wb") as f:
        f.write(struct.pack("<IHHIIHHI", 0x32434C55, bs, int(sizes.max()), len(bits), RATE, ch, kbps, 24) + payload)   # tools/ulc_Helper.h:10-20


@pytest.mark.skipif(not os.path.exists(TOOL), reason="ulc-codec_amd/ulcx-tool not built")
@pytest.mark.parametrize("fmt", ["FLOAT32", "PCM16"])
def test_tool_blocks_option_writes_the_bytes_of_the_full_decode(fmt, tmp_path):
    bs, ch, F, N = 2048, 2, 10, 20                           # (20 blocks: two range calls of the tool)
    files = []
    for i, (sid, nblk) in enumerate([(3, 40), (4, 40), (5, 24), (6, 11)]):
        blocks, bits, _ = oracle_stream(bs, ch, 50.0, sid)
        p = tmp_path / f"f{i}.ulc"
        _write_ulc(p, blocks[:nblk], bits[:nblk], bs, ch)
        files.append((p, nblk))
    full, part, part2 = tmp_path / "full", tmp_path / "part", tmp_path / "part2"
    for d in (full, part, part2):
        d.mkdir()
    names = [str(p) for p, _ in files]
    r = run_tool([TOOL, "decode", str(full), f"-format:{fmt}"] + names, check=False)
    assert r.returncode == 0, r.stderr.decode()
    r = run_tool([TOOL, "decode", str(part), f"-format:{fmt}", f"-blocks:{F},{N}"] + names, check=False)
    assert r.returncode == 0, r.stderr.decode()
    r = run_tool([TOOL, "decode", str(part2), f"-blocks:{F},{N}", f"-format:{fmt}", "-devices:2"] + names, check=False)
    assert r.returncode == 0, r.stderr.decode()
    bpf = ch * (4 if fmt == "FLOAT32" else 2) * bs             # bytes per block
    for p, nblk in files:
        want_full = open(full / (p.stem + ".wav"), "rb").read()
        got = open(part / (p.stem + ".wav"), "rb").read()
        n = min(N, nblk - F)                                   # trimmed where the file's header counts fewer blocks
        assert len(want_full) == 44 + nblk * bpf and len(got) == 44 + n * bpf, p.name
        assert got[44:] == want_full[44 + F * bpf:44 + (F + n) * bpf], f"{p.name}: -blocks:{F},{N} differs from the full decode's bytes"
        assert struct.unpack("<I", got[40:44])[0] == n * bpf and struct.unpack("<I", got[4:8])[0] == 36 + n * bpf, p.name
        assert got[8:40] == want_full[8:40], p.name            # the format chunk
        assert open(part2 / (p.stem + ".wav"), "rb").read() == got, f"{p.name}: -devices:2 changed the file"
    # a start at or past a file's block count: an error that names the file
    bad = tmp_path / "bad"
    bad.mkdir()
    r = run_tool([TOOL, "decode", str(bad), f"-blocks:11,4"] + names, check=False)
    assert r.returncode != 0 and "f3.ulc" in r.stderr.decode(), r.stderr.decode()
