"""Inputs and oracle references of the seek tests (tests/test_gpu_seek.py): packed payloads of oracle-encoded and of
hand-assembled streams, and what the oracle decoder says about them - block sizes, PCM, and the noise generator's state
in front of every block.  CPU only."""
import ctypes as C
import functools
import numpy as np
from ulc_testlib import oracle, ptr, f32p, i32p, u8p, synth_pcm, oracle_encode_debug, oracle_decode_stream, synth_block_stream

RATE = 44100
SEED0 = 1234567                                            # ulcDecoder.c:76
# (BlockSize, channels, VBR quality, synth_pcm stream id): oracle-encoded transient streams, 40 blocks each.  Every one has at
# least three window-switched blocks (the mono one with stream id 11: ids 3 .. 5 give two), and 39 of 40 blocks draw noise.
ORACLE_CASES = [(2048, 2, 50.0, 3), (4096, 2, 30.0, 3), (1024, 1, 20.0, 11), (2048, 3, 60.0, 3)]
ORACLE_BLOCKS = 40
# (BlockSize, channels): hand-assembled streams with every code of the syntax (synth_block_stream), 24 blocks each.  Seed 14:
# 24, 23 and 24 of the 24 blocks draw noise (with seed 11 the 512 x 1 stream has 21 such blocks, under the 90 % the index
# test asks of its inputs: a mono block of 512 often has no noise code at all).
SYNTH_CASES = [(2048, 2), (512, 1), (1024, 6)]
SYNTH_BLOCKS = 24
SYNTH_SEED = 14


@functools.lru_cache(maxsize=None)
def oracle_stream(bs, ch, q, sid, seed=11, n_blocks=ORACLE_BLOCKS):
    """-> (blocks uint8 [K][slot], bits [K], wc [K]) of an oracle-encoded transient stream."""
    pcm = synth_pcm(sid, n_blocks * bs, ch, RATE, transient=True, seed=seed)
    r = oracle_encode_debug(pcm, bs, RATE, 0, q, slot=2 * ch * bs + 16)
    return r["out"], r["bits"], r["wc"]


@functools.lru_cache(maxsize=None)
def synth_stream(bs, ch, seed=SYNTH_SEED, n_blocks=SYNTH_BLOCKS):
    """-> (blocks, bits) of a hand-assembled stream; the sizes are the oracle decoder's."""
    blocks, nbits = synth_block_stream(seed, n_blocks, ch, bs, 2 * ch * bs + 16)
    rc, _, bits = oracle_decode_stream(blocks, ch, bs)
    assert rc == 0 and np.array_equal(bits, nbits)
    return blocks, bits


def pack(streams, pad=64):
    """streams: [(blocks [K][slot], bits [K])] -> (payload uint8 [B][stride], payload_bytes int32 [B]): every block rounded
    up to a byte, no lengths stored (tools/ulcEncodeTool.c:160-169)."""
    pays = [b"".join(blk[k, :(int(bits[k]) + 7) // 8].tobytes() for k in range(len(bits))) for blk, bits in streams]
    stride = (max(len(p) for p in pays) + pad + 15) & ~15
    host = np.zeros((len(pays), stride), np.uint8)
    for s, p in enumerate(pays):
        host[s, :len(p)] = np.frombuffer(p, np.uint8)
    return host, np.array([len(p) for p in pays], np.int32)


def oracle_seeds(blocks, ch, bs):
    """Generator state in front of block k, k = 0 .. K (K: behind the last block): what orc_decode_stream_seeded hands back
    after decoding the first k blocks from the start state."""
    lib = oracle()
    lib.orc_decode_stream_seeded.argtypes = [C.c_int, C.c_int, u8p, C.c_int, C.c_int, f32p, i32p, C.POINTER(C.c_uint32)]
    K, slot = blocks.shape
    blocks = np.ascontiguousarray(blocks)
    pcm = np.zeros((K * bs, ch), np.float32)
    bits = np.zeros(K, np.int32)
    seeds = np.zeros(K + 1, np.uint32)
    seeds[0] = SEED0
    for k in range(1, K + 1):
        sd = C.c_uint32(SEED0)
        rc = lib.orc_decode_stream_seeded(ch, bs, ptr(blocks, u8p), slot, k, ptr(pcm, f32p), ptr(bits, i32p), C.byref(sd))
        assert rc == 0
        seeds[k] = sd.value
    return seeds


def damaged(payload, nbytes, seed):
    """A copy of a packed payload with ONE nybble overwritten by another value, at a seeded position inside the payload's
    first half."""
    rng = np.random.default_rng(seed)
    q = int(rng.integers(0, nbytes))                        # nybble number: [0, nbytes) is the first half of 2 * nbytes
    out = payload.copy()
    sh = 4 * (q & 1)
    old = (int(out[q >> 1]) >> sh) & 15
    new = (old + int(rng.integers(1, 16))) & 15
    out[q >> 1] = (int(out[q >> 1]) & ~(15 << sh)) | (new << sh)
    return out


def oracle_walk(payload, nbytes, ch, bs, max_blocks):
    """The oracle's decoder over a packed payload, block by block: every block's row is sliced from the payload (zeros behind
    its end, so a row never reads past the buffer) at the offset the oracle's own bit counts give, and the generator's state
    goes from block to block as in oracle_seeds.  It stops at the first block for which the oracle reports 0 bits, at the
    payload's end or after max_blocks.  -> (bits [n], byte offsets [n + 1], generator states [n + 1], inside): inside =
    every block walked ends inside the payload, i.e. no expected value comes from the zeros behind it."""
    lib = oracle()
    lib.orc_decode_stream_seeded.argtypes = [C.c_int, C.c_int, u8p, C.c_int, C.c_int, f32p, i32p, C.POINTER(C.c_uint32)]
    slot = 2 * ch * bs + 16
    padded = np.zeros(int(nbytes) + slot, np.uint8)
    padded[:nbytes] = payload[:nbytes]
    pcm = np.zeros((bs, ch), np.float32)
    b = np.zeros(1, np.int32)
    bits, offs, seeds, off, sd, inside = [], [0], [SEED0], 0, C.c_uint32(SEED0), True
    while len(bits) < max_blocks and off < nbytes:
        row = np.ascontiguousarray(padded[off:off + slot])
        b[0] = 0
        lib.orc_decode_stream_seeded(ch, bs, ptr(row, u8p), slot, 1, ptr(pcm, f32p), ptr(b, i32p), C.byref(sd))
        if b[0] == 0:
            break
        off += (int(b[0]) + 7) // 8
        inside = inside and off <= nbytes
        bits.append(int(b[0])); offs.append(off); seeds.append(sd.value)
    return np.array(bits, np.int32), np.array(offs, np.int64), np.array(seeds, np.uint32), inside


def oracle_pcm(blocks, ch, bs):
    """-> (pcm [K][bs][ch], bits [K]) of the oracle's sequential decode from block 0."""
    rc, pcm, bits = oracle_decode_stream(blocks, ch, bs)
    assert rc == 0
    return pcm.reshape(blocks.shape[0], bs, ch), bits


def expected_range(pcm, bits, first, n):
    """What a range call of n blocks from `first` must give: the slice of the sequential decode, zeros (0 bits) past the end."""
    K = pcm.shape[0]
    out = np.zeros((n,) + pcm.shape[1:], np.float32)
    ob = np.zeros(n, np.int32)
    m = max(0, min(n, K - first))
    out[:m] = pcm[first:first + m]
    ob[:m] = bits[first:first + m]
    return out, ob


def switched_starts(wc):
    """Starts directly behind a window-switched block (WindowCtrl other than the full-size, full-overlap 0x10)."""
    return [k + 1 for k in range(len(wc) - 1) if int(wc[k]) != 0x10]


def geometries():
    """The test streams grouped by decoder geometry: {(BlockSize, channels): [(name, blocks, bits, wc or None)]}."""
    g = {}
    for bs, ch, q, sid in ORACLE_CASES:
        blocks, bits, wc = oracle_stream(bs, ch, q, sid)
        g.setdefault((bs, ch), []).append((f"oracle {bs}x{ch} q{q:g}", blocks, bits, wc))
    for bs, ch in SYNTH_CASES:
        blocks, bits = synth_stream(bs, ch)
        g.setdefault((bs, ch), []).append((f"hand-assembled {bs}x{ch}", blocks, bits, None))
    return g
