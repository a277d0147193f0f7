"""The caller-buffer contract of include/ulc_amd.h ("Caller buffers"): every device-pointer entry, and every host form, is
called with ALL its buffers carved from one poisoned arena (tests/guarded_buffers.py) - each buffer at an odd multiple of
exactly the alignment the header states, between guards as large as the buffer would be at maxBlocksPerCall blocks - with
nBlocks below maxBlocksPerCall.  After the call: no guard byte changed, no input changed, and the defined extents of the
outputs equal the oracle bit for bit - over poison, so a byte the library owes and skips, ORs into or leaves to "the buffer
was zero anyway" differs.  Then: the same calls back to back on a stream with the inputs overwritten right behind each call,
and the refusal of misaligned pointers.

No case passes a pointer, size or index the header forbids; every store these tests look for lands inside the arena."""
import ctypes as C
import functools
import numpy as np
import pytest

from gpu_testlib import amd as _amd, dev as _dev, word
import guarded_buffers as gb
from ulc_testlib import synth_pcm, oracle_decode_stream, synth_block_stream, to_pcm16
from rates_testlib import OracleStream
from seek_testlib import oracle_stream, pack, oracle_seeds, oracle_pcm, expected_range

pytestmark = pytest.mark.gpu

# the alignments of include/ulc_amd.h, "Caller buffers" - these and no larger ones
A_PCM, A_PCM16, A_RATE, A_WORD, A_BYTE = 16, 8, 8, 4, 1
RATE = 44100
VBR50, CBR64 = (-50.0, 0.0), (64.0, 0.0)                    # settings in the tool's convention (rates_testlib.mode_of)
# (BlockSize, channels, streams, blocks per call, maxBlocksPerCall)
GEOMS = [(2048, 2, 5, 3, 5),                                # wave writer with direct packing, two-wave synthesis
         (2048, 1, 5, 3, 5),
         (512, 3, 5, 3, 5),                                 # unpaired channel, scalar loads
         (256, 2, 5, 3, 5),
         (4096, 2, 3, 3, 5),                                # k_select_pair
         (16384, 1, 2, 2, 3)]                               # k_xf_big, the general decoder kernel
CALLS = 2                                                   # consecutive calls per object: the second one starts from carried state


def _sync():
    import torch
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# references, computed once
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pcm(bs, ch, B, nblk):
    return np.stack([synth_pcm(s, nblk * bs, ch, RATE, transient=True, seed=bs + ch) for s in range(B)])     # [B][n][C]


@functools.lru_cache(maxsize=None)
def _oracle_enc(bs, ch, s, nblk, setting):
    """Per-block oracle results of stream s under one setting: [dict(bytes, bits, wc, cplx, ...)]."""
    x = synth_pcm(s, nblk * bs, ch, RATE, transient=True, seed=bs + ch)                                   # = _pcm(...)[s]
    o = OracleStream(ch, bs, RATE)
    r = [o.block(x[k * bs:(k + 1) * bs], setting) for k in range(nblk)]
    o.close()
    return r


def _table(B):
    """A per-stream table with all three modes."""
    t = [(-50.0, 0.0), (64.0, 0.0), (96.0, 0.3), (-70.0, 0.0), (48.0, 0.0)]
    return np.array([t[s % len(t)] for s in range(B)], np.float32)


def _scalar(g):
    """(mode, p0, p1) of the scalar API for a setting in the tool's convention."""
    return (0, -g[0], 0.0) if g[0] < 0 else (2, g[0], g[1]) if g[1] > 0 else (1, g[0], 0.0)


def _settings(B, what):
    """Per-stream settings of a scalar setting or a table."""
    if isinstance(what, tuple):
        return [what] * B
    return [(float(r), float(a)) for r, a in what]


def _check_encode(geom, what, k0, K, out, bits, wc, cplx, tag):
    bs, ch, B = geom[0], geom[1], geom[2]
    sets = _settings(B, what)
    for s in range(B):
        ref = _oracle_enc(bs, ch, s, CALLS * geom[3], sets[s])
        for k in range(K):
            r, t = ref[k0 + k], f"{tag}: stream {s} block {k0 + k}"
            if bits is not None:
                assert bits[s, k] == r["bits"], f"{t}: size {bits[s, k]} != {r['bits']}"
                nb = r["bits"] // 8
                assert np.array_equal(out[s, k, :nb], r["bytes"]), f"{t}: stream bytes differ"
            if wc is not None:
                assert wc[s, k] == r["wc"], f"{t}: WindowCtrl {wc[s, k]:#x} != {r['wc']:#x}"
            if cplx is not None:
                assert cplx[s, k].tobytes() == np.float32(r["cplx"]).tobytes(), f"{t}: BlockComplexity {cplx[s, k]} != {r['cplx']}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. encoder and analysis entries
# ---------------------------------------------------------------------------------------------------------------------
def _enc_arena(device, geom, slot, K, pcm16, R=1, tables=0, wc=True, cplx=True, out=True):
    bs, ch, B, _, maxK = geom
    esz = 2 if pcm16 else 4
    row = bs * ch * esz
    specs = [dict(name="d_pcm", nbytes=B * K * row, align=A_PCM16 if pcm16 else A_PCM, role="in", guard=B * maxK * row, row=row, rows_per_stream=K)]
    for t in range(tables):
        specs.append(dict(name=f"d_rate{t}", nbytes=8 * B, align=A_RATE, role="in", guard=8 * B * maxK, row=8, rows_per_stream=1))
    if out:
        specs.append(dict(name="d_out", nbytes=R * B * K * slot, align=A_BYTE, role="out", guard=B * maxK * slot, row=slot, rows_per_stream=K))
        specs.append(dict(name="d_bits", nbytes=R * B * K * 4, align=A_WORD, role="out", guard=B * maxK * 4, row=4, rows_per_stream=K))
    if wc:
        specs.append(dict(name="d_wc", nbytes=B * K * 4, align=A_WORD, role="out", guard=B * maxK * 4, row=4, rows_per_stream=K))
    if cplx:
        specs.append(dict(name="d_cplx", nbytes=B * K * 4, align=A_WORD, role="out", guard=B * maxK * 4, row=4, rows_per_stream=K))
    return gb.build(device, specs)


def _enc_call(amd, enc, geom, call, entry, what, wc=True, cplx=True, tag=""):
    """One guarded call of an encode / analyse entry on blocks [call*K, (call+1)*K); `what`: a scalar setting, a table, or a
    list of those (a ladder).  Checks guards, inputs and the defined extents against the oracle."""
    bs, ch, B, K, maxK = geom
    pcm16 = "pcm16" in entry
    analyse = entry.startswith("analyse")
    ladder = entry.endswith("ladder")
    rungs = what if ladder else [what]
    tabs = [g for g in rungs if not isinstance(g, tuple)] if not analyse else []
    R = len(rungs)
    a = _enc_arena(_dev(), geom, enc.slot, K, pcm16, R=R, tables=len(tabs), wc=wc, cplx=cplx, out=not analyse)
    x = _pcm(bs, ch, B, CALLS * K)[:, call * K * bs:(call + 1) * K * bs]
    a.load("d_pcm", to_pcm16(x) if pcm16 else x)          # exact: synth_pcm is on the PCM16 grid
    for t, g in enumerate(tabs):
        a.load(f"d_rate{t}", g)
    p = a.ptr
    d_wc, d_cplx = (p("d_wc") if wc else 0), (p("d_cplx") if cplx else 0)
    if analyse:
        enc.analyse_dev(p("d_pcm"), K, d_wc, d_cplx, pcm16=pcm16)
    elif ladder:
        arg, ti = [], 0
        for g in rungs:
            if isinstance(g, tuple):
                arg.append(_scalar(g))
            else:
                arg.append(p(f"d_rate{ti}")); ti += 1
        enc.encode_dev_ladder(arg, p("d_pcm"), K, p("d_out"), p("d_bits"), d_wc, d_cplx, pcm16=pcm16)
    elif tabs:
        enc.encode_dev_rates(p("d_rate0"), p("d_pcm"), K, p("d_out"), p("d_bits"), d_wc, d_cplx, pcm16=pcm16)
    else:
        mode, p0, p1 = _scalar(what)
        fn = enc.encode_dev_pcm16 if pcm16 else enc.encode_dev
        fn(p("d_pcm"), K, p("d_out"), p("d_bits"), d_wc, d_cplx, mode=mode, p0=p0, p1=p1)
    _sync()
    tag = f"{entry} {tag} bs={bs} ch={ch} call {call}"
    try:
        a.check()
    except gb.GuardError as e:
        raise AssertionError(f"{tag}: {e}") from None
    gwc = a.fetch("d_wc", np.int32).reshape(B, K) if wc else None
    gcx = a.fetch("d_cplx", np.float32).reshape(B, K) if cplx else None
    if analyse:
        _check_encode(geom, VBR50, call * K, K, None, None, gwc, gcx, tag)
        return
    out = a.fetch("d_out").reshape(R, B, K, enc.slot)
    bits = a.fetch("d_bits", np.int32).reshape(R, B, K)
    for r, g in enumerate(rungs):
        _check_encode(geom, g, call * K, K, out[r], bits[r], gwc, gcx, f"{tag} rung {r}")
    return out, bits


def _enc_run(geom, entry, what, nulls=("", ""), exact=0, tag=""):
    """Two consecutive calls of one entry on a fresh encoder; nulls: per call, which of d_wc / d_cplx is NULL ("w", "c", "wc")."""
    amd = _amd()
    bs, ch, B, K, maxK = geom
    enc = amd.BatchEncoder(B, ch, bs, RATE, maxK)
    if exact:
        enc.force_exact(exact)
    res = []
    for call in range(CALLS):
        res.append(_enc_call(amd, enc, geom, call, entry, what, wc="w" not in nulls[call], cplx="c" not in nulls[call], tag=tag))
    enc.close()
    return res


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_encode_entries_on_poisoned_guarded_buffers(geom):
    """ulcx_encode_dev / _dev_pcm16 under VBR 50 and CBR 64 (the probe passes of the rate search must leave d_out / d_bits of
    other blocks alone), the _rates forms with a table of all three modes, each once with d_wc and / or d_cplx NULL: the
    other outputs must not change (they are compared with the oracle either way, and with the all-outputs run)."""
    B = geom[2]
    full = _enc_run(geom, "encode_dev", VBR50, tag="VBR 50")
    part = _enc_run(geom, "encode_dev", VBR50, nulls=("wc", "c"), tag="VBR 50, d_wc / d_cplx NULL")
    for c in range(CALLS):
        for s in range(B):
            for k in range(geom[3]):
                nb = full[c][1][0, s, k] // 8
                assert part[c][1][0, s, k] == full[c][1][0, s, k] and np.array_equal(part[c][0][0, s, k, :nb], full[c][0][0, s, k, :nb])
    _enc_run(geom, "encode_dev", CBR64, nulls=("c", "w"), tag="CBR 64")
    _enc_run(geom, "encode_dev_pcm16", CBR64, tag="CBR 64")
    _enc_run(geom, "encode_dev_pcm16", VBR50, nulls=("w", "wc"), tag="VBR 50")
    _enc_run(geom, "encode_dev_rates", _table(B), nulls=("", "c"), tag="table")
    _enc_run(geom, "encode_dev_pcm16_rates", _table(B), nulls=("wc", ""), tag="table")


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_ladder_entries_on_poisoned_guarded_buffers(geom):
    """A 3-rung ladder with one table rung, float and PCM16 input: d_out [R][B][K][slot] / d_bits [R][B][K] of nBlocks blocks
    (a rung indexed with maxBlocksPerCall would land in the next rung or a guard), d_wc / d_cplx once, one call with each NULL."""
    rungs = [VBR50, _table(geom[2]), CBR64]
    _enc_run(geom, "encode_dev_ladder", rungs, nulls=("", "w"), tag="3 rungs")
    _enc_run(geom, "encode_dev_pcm16_ladder", rungs, nulls=("c", ""), tag="3 rungs")


@pytest.mark.parametrize("mode", [VBR50, CBR64], ids=["vbr", "cbr"])
def test_exact_path_packer_on_poisoned_guarded_buffers(mode):
    """force_exact(2): every second block of a call goes through the exact heapsort path and its packer; the same bytes."""
    _enc_run(GEOMS[0], "encode_dev", mode, exact=2, tag="force_exact(2)")


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_analyse_entries_on_poisoned_guarded_buffers(geom):
    """ulcx_analyse_dev / _dev_pcm16 with both outputs, with d_wc alone and with d_cplx alone."""
    _enc_run(geom, "analyse_dev", None, tag="wc + cplx")
    _enc_run(geom, "analyse_dev", None, nulls=("c", "w"), tag="one output")
    _enc_run(geom, "analyse_dev_pcm16", None, nulls=("", "c"), tag="pcm16")
    _enc_run(geom, "analyse_dev_pcm16", None, nulls=("w", ""), tag="pcm16")


# ---------------------------------------------------------------------------------------------------------------------
# 2. decoder entries, slot form
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_blocks(bs, ch, B, nblk):
    """Oracle-encoded VBR 50 blocks [B][nblk][wide slot] and their sizes in bytes."""
    wide = 2 * ch * bs + 16
    blocks = np.zeros((B, nblk, wide), np.uint8)
    nbytes = np.zeros((B, nblk), np.int64)
    for s in range(B):
        for k, r in enumerate(_oracle_enc(bs, ch, s, nblk, VBR50)):
            n = r["bits"] // 8
            blocks[s, k, :n] = r["bytes"]
            nbytes[s, k] = n
    return blocks, nbytes


def _expected_decode(blocks, ch, bs):
    """Oracle decode of [B][n][slot] -> (pcm [B][n][bs][ch], bits [B][n]); a stream the oracle rejects at block d is silent,
    with 0 bits, from d on."""
    B, n, _ = blocks.shape
    pcm = np.zeros((B, n, bs, ch), np.float32)
    bits = np.zeros((B, n), np.int32)
    dead = {}
    for s in range(B):
        rc, p, b = oracle_decode_stream(np.ascontiguousarray(blocks[s]), ch, bs)
        m = n if rc == 0 else rc - 1
        if rc != 0:
            dead[s] = m
        pcm[s, :m] = p.reshape(n, bs, ch)[:m]
        bits[s, :m] = b[:m]
    return pcm, bits, dead


def _dec_arena(device, B, K, maxK, bs, ch, slot, pcm16):
    esz = 2 if pcm16 else 4
    row = bs * ch * esz
    specs = [dict(name="d_in", nbytes=B * K * slot, align=A_BYTE, role="in", guard=B * maxK * slot, row=slot, rows_per_stream=K)]
    specs.append(dict(name="d_pcm", nbytes=B * K * row, align=A_PCM16 if pcm16 else A_PCM, role="out", guard=B * maxK * row, row=row, rows_per_stream=K))
    specs.append(dict(name="d_bits", nbytes=B * K * 4, align=A_WORD, role="out", guard=B * maxK * 4, row=4, rows_per_stream=K))
    return gb.build(device, specs)


def _corrupt_len(bs):
    """Bytes of 0x11 (zero runs of 50 coefficients, three nybbles each) that overrun a unit of any size up to bs."""
    return 38 if bs <= 2048 else bs // 16


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _first_diff(got, want):
    """(stream, block) of the first block that differs, for the message."""
    B, K = want.shape[:2]
    d = (got.reshape(B, K, -1).view(np.uint8) != want.reshape(B, K, -1).view(np.uint8)).any(axis=2)
    s, k = np.argwhere(d)[0]
    return f"first at stream {s} block {k} ({int(d.sum())} blocks differ)"


def _dec_slot_run(blocks, ch, bs, K, maxK, tag, cut=None, ref_blocks=None):
    """Slot-form decode of [B][calls*K][slot] in calls of K blocks, each call on its own arena whose d_in ends with the last
    slot's last byte; float and PCM16 output.  ref_blocks: the same blocks in slots the oracle may read to the end of."""
    amd = _amd()
    B, n, slot = blocks.shape
    want, wbits, dead = _expected_decode(blocks if ref_blocks is None else ref_blocks, ch, bs)
    for pcm16 in (False, True):
        dec = amd.BatchDecoder(B, ch, bs, maxK)
        for c in range(n // K):
            a = _dec_arena(_dev(), B, K, maxK, bs, ch, slot, pcm16)
            a.load("d_in", blocks[:, c * K:(c + 1) * K])
            fn = dec.decode_dev_pcm16 if pcm16 else dec.decode_dev
            fn(a.ptr("d_in"), slot, K, a.ptr("d_pcm"), a.ptr("d_bits"))
            _sync()
            t = f"{tag} {'pcm16' if pcm16 else 'float'} call {c}"
            try:
                a.check()
            except gb.GuardError as e:
                raise AssertionError(f"{t}: {e}") from None
            gbits = a.fetch("d_bits", np.int32).reshape(B, K)
            got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(B, K, bs, ch)
            w = want[:, c * K:(c + 1) * K]
            w = to_pcm16(w) if pcm16 else w
            assert np.array_equal(gbits, wbits[:, c * K:(c + 1) * K]), f"{t}: bits consumed differ: {_first_diff(gbits, wbits[:, c * K:(c + 1) * K])}"
            assert _same_bits(got, w), f"{t}: decoded samples differ (dead streams {dead} must be silent from there on): {_first_diff(got, w)}"
            if cut is not None:
                cut(dec.last_cut(), t)
        dec.close()


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_decode_entries_on_poisoned_guarded_buffers(geom):
    """ulcx_decode_dev / _dev_pcm16 on oracle-encoded streams, one of them with the 0x11 corruption in the middle of the first
    call: all of d_pcm / d_pcm16 is defined - zeros, over poison, for every block of the dead stream from its corrupt block
    on, in this call and the next."""
    bs, ch, B, K, maxK = geom
    blocks, _ = _oracle_blocks(bs, ch, B, CALLS * K)
    blocks = blocks.copy()
    blocks[1, 1, 2:2 + _corrupt_len(bs)] = 0x11             # long zero runs overrunning the subblock (ulcDecoder.c:127)
    want = _expected_decode(blocks, ch, bs)
    assert want[2] == {1: 1}, "the corruption must kill stream 1 at block 1"
    _dec_slot_run(blocks, ch, bs, K, maxK, f"oracle streams bs={bs} ch={ch}")


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2], GEOMS[3]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_decode_tight_slots_end_with_the_buffer(geom):
    """slotBytes = the largest block of the batch: slots are oddly aligned, the largest block fills its slot, and d_in ends
    exactly at the last slot's last byte, in front of a guard."""
    bs, ch, B, K, maxK = geom
    blocks, nbytes = _oracle_blocks(bs, ch, B, CALLS * K)
    slot = int(nbytes.max())
    tight = np.ascontiguousarray(blocks[:, :, :slot])
    assert (nbytes == slot).sum() >= 1
    _dec_slot_run(tight, ch, bs, K, maxK, f"tight slots of {slot} bytes bs={bs} ch={ch}", ref_blocks=blocks)


@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=lambda g: f"{g[0]}x{g[1]}")
def test_decode_hand_assembled_batch(geom):
    """Every code of the block syntax (synth_block_stream), the ones no encoder emits included."""
    bs, ch, B, K, maxK = geom
    slot = 2 * ch * bs + 16
    blocks = np.stack([synth_block_stream(4000 + 13 * s + bs, CALLS * K, ch, bs, slot)[0] for s in range(B)])
    assert not _expected_decode(blocks, ch, bs)[2]
    _dec_slot_run(blocks, ch, bs, K, maxK, f"hand-assembled bs={bs} ch={ch}")


def test_decode_even_cut_on_poisoned_guarded_buffers():
    """3 stereo streams x 40 blocks at BlockSize 1024: the synthesis is cut evenly over the device (ulcx_dec_split_plan), a
    workgroup enters a stream anywhere.  Stream 1 dies at block 11: the pieces behind it must write its silence themselves."""
    bs, ch, B, K, maxK = 1024, 2, 3, 40, 44
    blocks = np.stack([oracle_stream(bs, ch, 50.0, 3 + s, 11, K)[0] for s in range(B)]).copy()
    blocks[1, 11, 2:40] = 0x11
    assert _expected_decode(blocks, ch, bs)[2] == {1: 11}
    seen = []

    def cut(lc, t):
        grid, whole, resident = lc
        assert resident > 0 and grid > 0 and whole == 0, f"{t}: expected the even cut, got {grid} workgroups / {whole} whole streams ({resident} resident)"
        assert grid == _amd().lib().ulcx_dec_split_plan(B, K, resident)
        seen.append(grid)
    _dec_slot_run(blocks, ch, bs, K, maxK, "even cut 3 x 40", cut=cut)
    assert len(seen) == 2


# ---------------------------------------------------------------------------------------------------------------------
# 3. packed streams: pack, packed decode, index, range
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_streams_on_poisoned_guarded_buffers():
    """ulcx_pack_streams_dev: d_payload[s, :payloadBytes[s]] is the host concatenation, d_payloadBytes and d_maxBlock are
    written in full; with d_maxBlock NULL the rest is the same.  The rest of a payload row is not defined (the header)."""
    amd = _amd()
    bs, ch, B, K, maxK = GEOMS[0]
    blocks, nbytes = _oracle_blocks(bs, ch, B, CALLS * K)
    blocks, nbytes = blocks[:, :K], nbytes[:, :K]
    slot = blocks.shape[2]
    bits = (nbytes * 8).astype(np.int32)
    pays = [b"".join(blocks[s, k, :nbytes[s, k]].tobytes() for k in range(K)) for s in range(B)]
    stride = max(len(p) for p in pays) + 37                 # (an odd stride: rows start anywhere)
    for with_max in (True, False):
        specs = [dict(name="d_slots", nbytes=B * K * slot, align=A_BYTE, role="in", guard=B * maxK * slot, row=slot, rows_per_stream=K),
                 word("d_bits", B * K, "in", B * maxK, K),
                 dict(name="d_payload", nbytes=B * stride, align=A_BYTE, role="out", guard=B * maxK * slot, row=stride),
                 word("d_payloadBytes", B, "out")]
        if with_max:
            specs.append(word("d_maxBlock", B, "out"))
        a = gb.build(_dev(), specs)
        a.load("d_slots", blocks); a.load("d_bits", bits)
        rc = amd.lib().ulcx_pack_streams_dev(0, B, K, slot, a.ptr("d_slots"), a.ptr("d_bits"), a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"),
                                             a.ptr("d_maxBlock") if with_max else None, None)
        assert rc == 0
        _sync()
        a.check()
        pb = a.fetch("d_payloadBytes", np.int32)
        assert np.array_equal(pb, [len(p) for p in pays])
        pay = a.fetch("d_payload").reshape(B, stride)
        for s in range(B):
            assert pay[s, :pb[s]].tobytes() == pays[s], f"payload of stream {s} differs (d_maxBlock {'given' if with_max else 'NULL'})"
        if with_max:
            assert np.array_equal(a.fetch("d_maxBlock", np.int32), nbytes.max(axis=1))


@functools.lru_cache(maxsize=None)
def _seek_inputs(bs, ch, L, pad):
    """Four oracle streams of L blocks packed with `pad` bytes of stride behind the longest: (host, nbytes, [(pcm, bits)], [seeds])."""
    base = [oracle_stream(bs, ch, q, sid, 11, L) for q, sid in ((50.0, 3), (50.0, 4), (35.0, 5), (65.0, 6))]
    host, nb = pack([(blk, bits) for blk, bits, _ in base], pad=pad)
    return host, nb, [oracle_pcm(blk, ch, bs) for blk, _, _ in base], [oracle_seeds(blk, ch, bs) for blk, _, _ in base], [bits for _, bits, _ in base]


def _expected_index(B, L, maxB, nb4, bits4, seeds4, pick):
    import ulc_amd
    idx = np.zeros((B, maxB + 1), ulc_amd.INDEX_DTYPE)
    idx["ByteOffs"] = -1
    cnt = np.zeros(B, np.int32)
    for s in range(B):
        j = pick[s]
        offs = np.concatenate([[0], np.cumsum((bits4[j].astype(np.int64) + 7) // 8)])
        n = min(L, maxB)
        idx["ByteOffs"][s, :n + 1] = offs[:n + 1]
        idx["RngState"][s, :n + 1] = seeds4[j][:n + 1]
        cnt[s] = n
    return idx, cnt


def test_packed_decode_and_index_on_poisoned_guarded_buffers():
    """ulcx_decode_packed_dev (two calls, the read position carried) and ulcx_index_packed_dev with maxBlocks beyond the
    streams' end: all [nStreams][maxBlocks+1] entries are defined, the {-1, 0} ones behind the closing entry included.  The
    payload buffer ends with the last stream's stride; one stream's payload is cut short, so it ends inside a call."""
    amd = _amd()
    bs, ch, B, K, maxK, L = 2048, 2, 5, 3, 5, 6
    host4, nb4, refs, seeds4, bits4 = _seek_inputs(bs, ch, L, 0)
    pick = np.arange(B) % 4
    host, nbytes = np.ascontiguousarray(host4[pick]), nb4[pick].copy()
    stride = host.shape[1]
    offs1 = np.concatenate([[0], np.cumsum((bits4[1].astype(np.int64) + 7) // 8)])
    nbytes[1] = offs1[4] + 9                                # stream 1 ends 9 bytes into its block 4: four whole blocks
    row = bs * ch * 4
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    for c in range(2):
        a = gb.build(_dev(), [dict(name="d_payload", nbytes=B * stride, align=A_BYTE, role="in", guard=B * stride, row=stride),
                              word("d_payloadBytes", B, "in"),
                              dict(name="d_pcm", nbytes=B * K * row, align=A_PCM, role="out", guard=B * maxK * row, row=row, rows_per_stream=K),
                              word("d_bits", B * K, "out", B * maxK, K)])
        a.load("d_payload", host); a.load("d_payloadBytes", nbytes)
        dec.decode_packed_dev(a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"), K, a.ptr("d_pcm"), a.ptr("d_bits"))
        _sync()
        a.check()
        got = a.fetch("d_pcm", np.float32).reshape(B, K, bs, ch)
        gb_ = a.fetch("d_bits", np.int32).reshape(B, K)
        for s in range(B):
            p, b = refs[pick[s]]
            p, b = (p[:4], b[:4]) if s == 1 else (p, b)
            want, wb = expected_range(p, b, c * K, K)
            assert np.array_equal(gb_[s], wb), f"packed call {c} stream {s}: bits {gb_[s]} != {wb}"
            assert _same_bits(got[s], want), f"packed call {c} stream {s}: samples differ (a stream past its end must be silent)"
    # index: maxBlocks = L + 3
    maxB = L + 3
    a = gb.build(_dev(), [dict(name="d_payload", nbytes=B * stride, align=A_BYTE, role="in", guard=B * stride, row=stride),
                          word("d_payloadBytes", B, "in"),
                          dict(name="d_index", nbytes=8 * B * (maxB + 1), align=A_WORD, role="out", guard=8 * B * (maxB + 1), row=8, rows_per_stream=maxB + 1),
                          word("d_nBlocks", B, "out")])
    a.load("d_payload", host); a.load("d_payloadBytes", nbytes)
    dec.index_packed_dev(a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"), maxB, a.ptr("d_index"), a.ptr("d_nBlocks"))
    _sync()
    a.check()
    widx, wcnt = _expected_index(B, L, maxB, nb4, bits4, seeds4, pick)
    wcnt[1] = 4
    widx["ByteOffs"][1, 5:] = -1; widx["RngState"][1, 5:] = 0
    gidx = a.fetch("d_index", amd.INDEX_DTYPE).reshape(B, maxB + 1)
    assert np.array_equal(a.fetch("d_nBlocks", np.int32), wcnt)
    assert np.array_equal(gidx, widx), f"index differs in streams {sorted(set(np.argwhere(gidx != widx)[:, 0].tolist()))}"
    dec.close()


def _range_call(amd, dec, host, nbytes, index, count, first, N, maxK, bs, ch, pcm16):
    B, stride = host.shape
    esz = 2 if pcm16 else 4
    row = bs * ch * esz
    istride = index.shape[1]
    a = gb.build(_dev(), [dict(name="d_payload", nbytes=B * stride, align=A_BYTE, role="in", guard=B * stride, row=stride),
                          word("d_payloadBytes", B, "in"),
                          dict(name="d_index", nbytes=8 * B * istride, align=A_WORD, role="in", guard=8 * B * istride, row=8, rows_per_stream=istride),
                          word("d_indexBlocks", B, "in"), word("d_first", B, "in"),
                          dict(name="d_pcm", nbytes=B * N * row, align=A_PCM16 if pcm16 else A_PCM, role="out", guard=B * maxK * row, row=row, rows_per_stream=N),
                          word("d_bits", B * N, "out", B * maxK, N)])
    a.load("d_payload", host); a.load("d_payloadBytes", nbytes); a.load("d_index", index); a.load("d_indexBlocks", count); a.load("d_first", first)
    dec.decode_range_dev(a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"), a.ptr("d_index"), istride, a.ptr("d_indexBlocks"), a.ptr("d_first"), N,
                         a.ptr("d_pcm"), a.ptr("d_bits"), pcm16=pcm16)
    _sync()
    a.check()
    return a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(B, N, bs, ch), a.fetch("d_bits", np.int32).reshape(B, N)


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_range_entries_on_poisoned_guarded_buffers(pcm16):
    """ulcx_decode_range_dev / _dev_pcm16: 3 blocks of a decoder of 5 per call, from the start, from inside, running past the end
    (0 bits and silence over poison), and from outside the index (a stream of 0 bits)."""
    amd = _amd()
    bs, ch, B, N, maxK, L = 2048, 2, 5, 3, 5, 6
    host4, nb4, refs, seeds4, bits4 = _seek_inputs(bs, ch, L, 0)
    pick = np.arange(B) % 4
    host, nbytes = np.ascontiguousarray(host4[pick]), nb4[pick].copy()
    index, count = _expected_index(B, L, L, nb4, bits4, seeds4, pick)
    first = np.array([0, 2, 5, 3, L + 1], np.int32)        # stream 2 runs past its end, stream 4 starts outside its index
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    got, gbits = _range_call(amd, dec, host, nbytes, index, count, first, N, maxK, bs, ch, pcm16)
    dec.close()
    for s in range(B):
        p, b = refs[pick[s]]
        want, wb = expected_range(p, b, int(first[s]), N) if first[s] <= L else (np.zeros((N, bs, ch), np.float32), np.zeros(N, np.int32))
        want = to_pcm16(want) if pcm16 else want
        assert np.array_equal(gbits[s], wb), f"stream {s} from block {first[s]}: bits {gbits[s]} != {wb}"
        assert _same_bits(got[s], want), f"stream {s} from block {first[s]}: samples differ"


def test_range_tail_cut_on_poisoned_guarded_buffers():
    """The cut of the last round (ulcx_dec_range_tail_plan) at the smallest geometry with a resident count, stereo BlockSize 256:
    resident + 2 * resident // 3 streams, the shortest call the plan cuts (6 blocks, pieces of 2), PCM16 output.  The call must
    report that cut - otherwise this case tests nothing - and every stream equals the oracle's slice."""
    amd = _amd()
    bs, ch, N, maxK, L = 256, 2, 6, 7, 12
    probe = amd.BatchDecoder(8, ch, bs, maxK)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0, "stereo BlockSize 256 runs the two-wave synthesis kernel"
    B = resident + 2 * resident // 3
    full = C.c_int32(0)
    tail = amd.lib().ulcx_dec_range_tail_plan(B, N, resident, C.byref(full))
    assert tail > 0 and full.value == resident, (B, resident, tail, full.value)
    host4, nb4, refs, seeds4, bits4 = _seek_inputs(bs, ch, L, 0)
    pick = np.arange(B) % 4
    host, nbytes = np.ascontiguousarray(host4[pick]), nb4[pick].copy()
    index, count = _expected_index(B, L, L, nb4, bits4, seeds4, pick)
    first = np.random.default_rng(31).integers(0, L - N + 1, B).astype(np.int32)
    first[0], first[resident], first[B - 1] = 0, 0, L - N + 2      # the last stream runs past its end
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    got, gbits = _range_call(amd, dec, host, nbytes, index, count, first, N, maxK, bs, ch, True)
    grid, whole, res2 = dec.last_cut()
    dec.close()
    assert (grid, whole) == (full.value + tail, full.value), f"the tail cut was not taken: {grid} workgroups, {whole} whole streams ({res2} resident, plan {tail})"
    # expected, per (base stream, start): computed once and gathered
    want = np.zeros((B, N, bs, ch), np.int16)
    wbits = np.zeros((B, N), np.int32)
    for j in range(4):
        for f in range(L + 1):
            sel = np.flatnonzero((pick == j) & (first == f))
            if sel.size:
                w, b = expected_range(refs[j][0], refs[j][1], f, N)
                want[sel], wbits[sel] = to_pcm16(w), b
    assert np.array_equal(gbits, wbits), f"bits differ: {_first_diff(gbits, wbits)}"
    assert _same_bits(got, want), f"samples differ: {_first_diff(got, want)}"


# ---------------------------------------------------------------------------------------------------------------------
# 4. host forms: the same check with a numpy arena; they must copy back exactly the [nBlocks] extents
# ---------------------------------------------------------------------------------------------------------------------
def _hp(addr, t):
    return C.cast(C.c_void_p(addr), t)


def test_host_forms_copy_back_exactly_their_extents():
    """ulcx_encode_host / _host_rates / _host_ladder, ulcx_analyse_host, ulcx_decode_host, ulcx_decode_packed_host,
    ulcx_index_packed_host and ulcx_decode_range_host on host buffers carved from one poisoned numpy arena each, 3 blocks of
    an object of 5 per call: the internal staging is sized for 5, the copies back must stop at 3."""
    amd = _amd()
    L = amd.lib()
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    geom = GEOMS[0]
    bs, ch, B, K, maxK = geom
    row = bs * ch * 4
    x = _pcm(bs, ch, B, CALLS * K)[:, :K * bs]
    enc = amd.BatchEncoder(B, ch, bs, RATE, maxK)
    slot = enc.slot

    def enc_specs(R, tables=0):
        sp = [dict(name="h_pcm", nbytes=B * K * row, align=4, role="in", guard=B * maxK * row, row=row, rows_per_stream=K)]
        sp += [dict(name=f"h_rate{t}", nbytes=8 * B, align=4, role="in", row=8) for t in range(tables)]
        sp += [dict(name="h_out", nbytes=R * B * K * slot, align=1, role="out", guard=B * maxK * slot, row=slot, rows_per_stream=K),
               word("h_bits", R * B * K, "out", B * maxK, K), word("h_wc", B * K, "out", B * maxK, K), word("h_cplx", B * K, "out", B * maxK, K)]
        return sp

    def enc_check(a, R, whats, tag):
        a.check()
        out = a.fetch("h_out").reshape(R, B, K, slot); bits = a.fetch("h_bits", np.int32).reshape(R, B, K)
        wc = a.fetch("h_wc", np.int32).reshape(B, K); cx = a.fetch("h_cplx", np.float32).reshape(B, K)
        for r, g in enumerate(whats):
            _check_encode(geom, g, 0, K, out[r], bits[r], wc, cx, f"{tag} rung {r}")

    a = gb.build(None, enc_specs(1)); a.load("h_pcm", x)
    assert L.ulcx_encode_host(enc.h, 1, 64.0, 0.0, _hp(a.ptr("h_pcm"), f32p), K, _hp(a.ptr("h_out"), u8p), _hp(a.ptr("h_bits"), i32p),
                              _hp(a.ptr("h_wc"), i32p), _hp(a.ptr("h_cplx"), f32p)) == 0
    enc_check(a, 1, [CBR64], "ulcx_encode_host CBR 64")
    enc.reset()
    tab = _table(B)
    a = gb.build(None, enc_specs(1, 1)); a.load("h_pcm", x); a.load("h_rate0", tab)
    assert L.ulcx_encode_host_rates(enc.h, _hp(a.ptr("h_rate0"), f32p), _hp(a.ptr("h_pcm"), f32p), K, _hp(a.ptr("h_out"), u8p), _hp(a.ptr("h_bits"), i32p),
                                    _hp(a.ptr("h_wc"), i32p), _hp(a.ptr("h_cplx"), f32p)) == 0
    enc_check(a, 1, [tab], "ulcx_encode_host_rates")
    enc.reset()
    a = gb.build(None, enc_specs(3, 1)); a.load("h_pcm", x); a.load("h_rate0", tab)
    rungs = (amd.Rung * 3)()
    rungs[0].mode, rungs[0].param0 = 0, 50.0
    rungs[1].rate = a.ptr("h_rate0")
    rungs[2].mode, rungs[2].param0 = 1, 64.0
    assert L.ulcx_encode_host_ladder(enc.h, rungs, 3, _hp(a.ptr("h_pcm"), f32p), K, _hp(a.ptr("h_out"), u8p), _hp(a.ptr("h_bits"), i32p),
                                     _hp(a.ptr("h_wc"), i32p), _hp(a.ptr("h_cplx"), f32p)) == 0
    enc_check(a, 3, [VBR50, tab, CBR64], "ulcx_encode_host_ladder")
    enc.reset()
    a = gb.build(None, [enc_specs(1)[0], word("h_wc", B * K, "out", B * maxK, K), word("h_cplx", B * K, "out", B * maxK, K)])
    a.load("h_pcm", x)
    assert L.ulcx_analyse_host(enc.h, _hp(a.ptr("h_pcm"), f32p), K, _hp(a.ptr("h_wc"), i32p), _hp(a.ptr("h_cplx"), f32p)) == 0
    a.check()
    _check_encode(geom, VBR50, 0, K, None, None, a.fetch("h_wc", np.int32).reshape(B, K), a.fetch("h_cplx", np.float32).reshape(B, K), "ulcx_analyse_host")
    enc.close()

    # decoder, slot form: one stream dies in the middle of the call
    blocks, _ = _oracle_blocks(bs, ch, B, CALLS * K)
    blocks = blocks[:, :K].copy()
    blocks[1, 1, 2:40] = 0x11
    want, wbits, dead = _expected_decode(blocks, ch, bs)
    assert dead == {1: 1}
    wslot = blocks.shape[2]
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    pcm_spec = dict(name="h_pcm", nbytes=B * K * row, align=4, role="out", guard=B * maxK * row, row=row, rows_per_stream=K)
    a = gb.build(None, [dict(name="h_in", nbytes=B * K * wslot, align=1, role="in", guard=B * maxK * wslot, row=wslot, rows_per_stream=K), pcm_spec,
                        word("h_bits", B * K, "out", B * maxK, K)])
    a.load("h_in", blocks)
    assert L.ulcx_decode_host(dec.h, _hp(a.ptr("h_in"), u8p), wslot, K, _hp(a.ptr("h_pcm"), f32p), _hp(a.ptr("h_bits"), i32p)) == 0
    a.check()
    assert np.array_equal(a.fetch("h_bits", np.int32).reshape(B, K), wbits) and _same_bits(a.fetch("h_pcm", np.float32).reshape(B, K, bs, ch), want), "ulcx_decode_host"
    dec.close()

    # packed forms
    Ls = 6
    host4, nb4, refs, seeds4, bits4 = _seek_inputs(bs, ch, Ls, 0)
    pick = np.arange(B) % 4
    host, nbytes = np.ascontiguousarray(host4[pick]), nb4[pick].copy()
    stride = host.shape[1]
    pay_specs = [dict(name="h_payload", nbytes=B * stride, align=1, role="in", guard=B * stride, row=stride), word("h_payloadBytes", B, "in")]
    dec = amd.BatchDecoder(B, ch, bs, maxK)
    a = gb.build(None, pay_specs + [pcm_spec, word("h_bits", B * K, "out", B * maxK, K)])
    a.load("h_payload", host); a.load("h_payloadBytes", nbytes)
    assert L.ulcx_decode_packed_host(dec.h, _hp(a.ptr("h_payload"), u8p), stride, _hp(a.ptr("h_payloadBytes"), i32p), K, _hp(a.ptr("h_pcm"), f32p),
                                     _hp(a.ptr("h_bits"), i32p)) == 0
    a.check()
    got, gbits = a.fetch("h_pcm", np.float32).reshape(B, K, bs, ch), a.fetch("h_bits", np.int32).reshape(B, K)
    for s in range(B):
        w, b = expected_range(refs[pick[s]][0], refs[pick[s]][1], 0, K)
        assert np.array_equal(gbits[s], b) and _same_bits(got[s], w), f"ulcx_decode_packed_host stream {s}"
    maxB = Ls + 2
    a = gb.build(None, pay_specs + [dict(name="h_index", nbytes=8 * B * (maxB + 1), align=4, role="out", guard=8 * B * (maxB + 1), row=8, rows_per_stream=maxB + 1),
                                    word("h_nBlocks", B, "out")])
    a.load("h_payload", host); a.load("h_payloadBytes", nbytes)
    assert L.ulcx_index_packed_host(dec.h, _hp(a.ptr("h_payload"), u8p), stride, _hp(a.ptr("h_payloadBytes"), i32p), maxB, C.c_void_p(a.ptr("h_index")),
                                    _hp(a.ptr("h_nBlocks"), i32p)) == 0
    a.check()
    widx, wcnt = _expected_index(B, Ls, maxB, nb4, bits4, seeds4, pick)
    assert np.array_equal(a.fetch("h_nBlocks", np.int32), wcnt) and np.array_equal(a.fetch("h_index", amd.INDEX_DTYPE).reshape(B, maxB + 1), widx), "ulcx_index_packed_host"
    first = np.array([0, 2, 5, 3, 1], np.int32)
    a = gb.build(None, pay_specs + [dict(name="h_index", nbytes=8 * B * (maxB + 1), align=4, role="in", row=8, rows_per_stream=maxB + 1),
                                    word("h_indexBlocks", B, "in"), word("h_first", B, "in"), pcm_spec, word("h_bits", B * K, "out", B * maxK, K)])
    a.load("h_payload", host); a.load("h_payloadBytes", nbytes); a.load("h_index", widx); a.load("h_indexBlocks", wcnt); a.load("h_first", first)
    assert L.ulcx_decode_range_host(dec.h, _hp(a.ptr("h_payload"), u8p), stride, _hp(a.ptr("h_payloadBytes"), i32p), C.c_void_p(a.ptr("h_index")), maxB + 1,
                                    _hp(a.ptr("h_indexBlocks"), i32p), _hp(a.ptr("h_first"), i32p), K, _hp(a.ptr("h_pcm"), f32p), _hp(a.ptr("h_bits"), i32p)) == 0
    a.check()
    got, gbits = a.fetch("h_pcm", np.float32).reshape(B, K, bs, ch), a.fetch("h_bits", np.int32).reshape(B, K)
    for s in range(B):
        w, b = expected_range(refs[pick[s]][0], refs[pick[s]][1], int(first[s]), K)
        assert np.array_equal(gbits[s], b) and _same_bits(got[s], w), f"ulcx_decode_range_host stream {s} from block {first[s]}"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. stream order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["vbr", "ladder", "analyse", "decode"])
def test_inputs_may_be_overwritten_right_behind_the_call_on_its_stream(what):
    """Two calls back to back on a torch.cuda.Stream, no host synchronisation in between: copy the input into the carved
    region, call, copy the outputs away and overwrite the input region with poison - all on that stream - then the same with
    the next blocks, then one synchronisation.  Both calls' saved outputs must equal the oracle, the state carried between the
    calls included.  The library forks onto private side streams (window control reads the caller's PCM there): a side stream
    not joined before the call returns lets the poison, or the second call's input, reach a kernel of the first.
    A pass cannot prove that no such race exists - the overwrite may simply lose it; a failure is a real finding."""
    import torch
    amd = _amd()
    dev = _dev()
    geom = GEOMS[0]
    bs, ch, B, K, maxK = geom
    st = torch.cuda.Stream(device=dev)
    R = 2 if what == "ladder" else 1
    rungs = [VBR50, CBR64][:R]
    if what == "decode":
        blocks, _ = _oracle_blocks(bs, ch, B, CALLS * K)
        slot = blocks.shape[2]
        obj = amd.BatchDecoder(B, ch, bs, maxK)
        a = _dec_arena(dev, B, K, maxK, bs, ch, slot, False)
        inp, src = "d_in", [torch.from_numpy(np.ascontiguousarray(blocks[:, c * K:(c + 1) * K])).to(dev).reshape(-1) for c in range(CALLS)]
        outs = ["d_pcm", "d_bits"]
    else:
        obj = amd.BatchEncoder(B, ch, bs, RATE, maxK)
        slot = obj.slot
        a = _enc_arena(dev, geom, slot, K, False, R=R, out=what != "analyse")
        x = _pcm(bs, ch, B, CALLS * K)
        inp, src = "d_pcm", [torch.from_numpy(np.ascontiguousarray(x[:, c * K * bs:(c + 1) * K * bs])).to(dev).reshape(-1).view(torch.uint8) for c in range(CALLS)]
        outs = (["d_out", "d_bits"] if what != "analyse" else []) + ["d_wc", "d_cplx"]
    poison = a.poison_of(inp)
    dst = a.view(inp)
    saved = [{n: torch.empty_like(a.view(n)) for n in outs} for _ in range(CALLS)]
    torch.cuda.synchronize()                                 # everything above is in place; from here on only the stream orders
    p = a.ptr
    with torch.cuda.stream(st):
        for c in range(CALLS):
            dst.copy_(src[c], non_blocking=True)                                        # 1
            if what == "decode":                                                        # 2
                obj.decode_dev(p("d_in"), slot, K, p("d_pcm"), p("d_bits"), stream=st.cuda_stream)
            elif what == "analyse":
                obj.analyse_dev(p("d_pcm"), K, p("d_wc"), p("d_cplx"), stream=st.cuda_stream)
            elif what == "ladder":
                obj.encode_dev_ladder([(0, 50.0, 0.0), (1, 64.0, 0.0)], p("d_pcm"), K, p("d_out"), p("d_bits"), p("d_wc"), p("d_cplx"), stream=st.cuda_stream)
            else:
                obj.encode_dev(p("d_pcm"), K, p("d_out"), p("d_bits"), p("d_wc"), p("d_cplx"), mode=0, p0=50.0, stream=st.cuda_stream)
            for n in outs:                                                              # 3
                saved[c][n].copy_(a.view(n), non_blocking=True)
            dst.copy_(poison, non_blocking=True)
    st.synchronize()                                                                    # 5
    a.expect(inp, poison.cpu().numpy())                      # (the input region must hold the pattern again)
    a.check()
    wall = _expected_decode(blocks, ch, bs) if what == "decode" else None
    for c in range(CALLS):
        h = {n: saved[c][n].cpu().numpy() for n in outs}
        tag = f"{what} on a stream, call {c}"
        if what == "decode":
            want, wbits = wall[0][:, c * K:(c + 1) * K], wall[1][:, c * K:(c + 1) * K]
            assert np.array_equal(h["d_bits"].view(np.int32).reshape(B, K), wbits), f"{tag}: bits consumed differ"
            assert _same_bits(h["d_pcm"].view(np.float32).reshape(B, K, bs, ch), want), f"{tag}: decoded samples differ"
            continue
        wc, cx = h["d_wc"].view(np.int32).reshape(B, K), h["d_cplx"].view(np.float32).reshape(B, K)
        if what == "analyse":
            _check_encode(geom, VBR50, c * K, K, None, None, wc, cx, tag)
            continue
        out, bits = h["d_out"].reshape(R, B, K, slot), h["d_bits"].view(np.int32).reshape(R, B, K)
        for r, g in enumerate(rungs):
            _check_encode(geom, g, c * K, K, out[r], bits[r], wc, cx, f"{tag} rung {r}")
    obj.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. misaligned pointers are refused
# ---------------------------------------------------------------------------------------------------------------------
def test_misaligned_pointers_are_refused_and_leave_the_state_untouched():
    """Every _dev entry returns ULCX_ERR_ARG for a pointer off the alignment the header states, before any device work: two
    objects run the same valid calls, one of them with refused calls in between, and stay bit for bit alike (and equal to the
    oracle).  The refused pointers are valid addresses inside buffers the test owns, only misaligned; none reaches a kernel."""
    import torch
    amd = _amd()
    dev = _dev()
    geom = GEOMS[0]
    bs, ch, B, K, maxK = geom
    x = _pcm(bs, ch, B, CALLS * K)
    encs = [amd.BatchEncoder(B, ch, bs, RATE, maxK) for _ in range(2)]
    slot = encs[0].slot
    tab = torch.from_numpy(_table(B)).to(dev)
    t = lambda *shape, dtype=torch.uint8: torch.empty(*shape, dtype=dtype, device=dev)
    spare = {k: t(1 << 20) for k in ("pcm", "out", "bits", "wc", "cplx", "pay", "idx", "cnt", "first", "nb")}
    P = {k: v.data_ptr() for k, v in spare.items()}
    for v in P.values():
        assert v % 256 == 0
    rate = tab.data_ptr()
    outs = []
    for c in range(CALLS):
        got = []
        for i, enc in enumerate(encs):
            if i == 0 and c == 1:
                bad = [
                    lambda: enc.encode_dev(P["pcm"] + 8, K, P["out"], P["bits"], P["wc"], P["cplx"]),
                    lambda: enc.encode_dev(P["pcm"] + 4, K, P["out"], P["bits"]),
                    lambda: enc.encode_dev(P["pcm"], K, P["out"], P["bits"] + 2),
                    lambda: enc.encode_dev(P["pcm"], K, P["out"], P["bits"], P["wc"] + 1),
                    lambda: enc.encode_dev(P["pcm"], K, P["out"], P["bits"], 0, P["cplx"] + 2),
                    lambda: enc.encode_dev_pcm16(P["pcm"] + 4, K, P["out"], P["bits"]),
                    lambda: enc.encode_dev_pcm16(P["pcm"] + 2, K, P["out"], P["bits"], mode=1, p0=64.0),
                    lambda: enc.encode_dev_rates(rate + 4, P["pcm"], K, P["out"], P["bits"]),
                    lambda: enc.encode_dev_rates(rate, P["pcm"] + 8, K, P["out"], P["bits"]),
                    lambda: enc.encode_dev_rates(rate, P["pcm"] + 4, K, P["out"], P["bits"], pcm16=True),
                    lambda: enc.encode_dev_ladder([(0, 50.0, 0.0), rate + 4], P["pcm"], K, P["out"], P["bits"]),
                    lambda: enc.encode_dev_ladder([(0, 50.0, 0.0), rate], P["pcm"] + 8, K, P["out"], P["bits"]),
                    lambda: enc.encode_dev_ladder([(0, 50.0, 0.0)], P["pcm"] + 4, K, P["out"], P["bits"], pcm16=True),
                    lambda: enc.encode_dev_ladder([(0, 50.0, 0.0)], P["pcm"], K, P["out"], P["bits"] + 2),
                    lambda: enc.analyse_dev(P["pcm"] + 8, K, P["wc"], P["cplx"]),
                    lambda: enc.analyse_dev(P["pcm"] + 4, K, P["wc"], P["cplx"], pcm16=True),
                    lambda: enc.analyse_dev(P["pcm"], K, P["wc"] + 2, 0),
                    lambda: enc.analyse_dev(P["pcm"], K, 0, P["cplx"] + 1),
                ]
                for call in bad:
                    with pytest.raises(amd.UlcError, match=r"\(-1\).*not aligned"):
                        call()
            o, b, w, cx = t(B, K, slot), t(B, K, dtype=torch.int32), t(B, K, dtype=torch.int32), t(B, K, dtype=torch.float32)
            d_pcm = torch.from_numpy(np.ascontiguousarray(x[:, c * K * bs:(c + 1) * K * bs])).to(dev)
            enc.encode_dev(d_pcm.data_ptr(), K, o.data_ptr(), b.data_ptr(), w.data_ptr(), cx.data_ptr(), mode=1, p0=64.0)
            torch.cuda.synchronize()
            got.append((o.cpu().numpy(), b.cpu().numpy(), w.cpu().numpy(), cx.cpu().numpy()))
            _check_encode(geom, CBR64, c * K, K, *got[-1], f"encoder {i} call {c}")
        outs.append(got)
    for enc in encs:
        enc.close()
    # decoder side
    blocks, _ = _oracle_blocks(bs, ch, B, CALLS * K)
    wslot = blocks.shape[2]
    want, wbits, _ = _expected_decode(blocks, ch, bs)
    L = amd.lib()
    decs = [amd.BatchDecoder(B, ch, bs, maxK) for _ in range(2)]
    for c in range(CALLS):
        for i, dec in enumerate(decs):
            if i == 0 and c == 1:
                rng = lambda **kw: dec.decode_range_dev(kw.get("pay", P["pay"]), 4096, kw.get("nb", P["nb"]), kw.get("idx", P["idx"]), 8, kw.get("cnt", P["cnt"]),
                                                        kw.get("first", P["first"]), K, kw.get("pcm", P["pcm"]), kw.get("bits", P["bits"]), pcm16=kw.get("pcm16", False))
                bad = [
                    lambda: dec.decode_dev(P["out"], wslot, K, P["pcm"] + 8, P["bits"]),
                    lambda: dec.decode_dev(P["out"], wslot, K, P["pcm"], P["bits"] + 2),
                    lambda: dec.decode_dev_pcm16(P["out"], wslot, K, P["pcm"] + 4, P["bits"]),
                    lambda: dec.decode_packed_dev(P["pay"], 4096, P["nb"] + 2, K, P["pcm"], P["bits"]),
                    lambda: dec.decode_packed_dev(P["pay"], 4096, P["nb"], K, P["pcm"] + 4, P["bits"]),
                    lambda: dec.decode_packed_dev(P["pay"], 4096, P["nb"], K, P["pcm"], P["bits"] + 1),
                    lambda: dec.index_packed_dev(P["pay"], 4096, P["nb"] + 2, 8, P["idx"], P["cnt"]),
                    lambda: dec.index_packed_dev(P["pay"], 4096, P["nb"], 8, P["idx"] + 2, P["cnt"]),
                    lambda: dec.index_packed_dev(P["pay"], 4096, P["nb"], 8, P["idx"], P["cnt"] + 1),
                    lambda: rng(nb=P["nb"] + 2), lambda: rng(idx=P["idx"] + 2), lambda: rng(cnt=P["cnt"] + 1), lambda: rng(first=P["first"] + 2),
                    lambda: rng(pcm=P["pcm"] + 8), lambda: rng(bits=P["bits"] + 2), lambda: rng(pcm=P["pcm"] + 4, pcm16=True),
                ]
                for call in bad:
                    with pytest.raises(amd.UlcError, match=r"\(-1\).*not aligned"):
                        call()
                for args in ((P["bits"] + 2, P["nb"], P["cnt"]), (P["bits"], P["nb"] + 2, P["cnt"]), (P["bits"], P["nb"], P["cnt"] + 1)):
                    assert L.ulcx_pack_streams_dev(0, B, K, wslot, P["out"], args[0], P["pay"], 1 << 16, args[1], args[2], None) == -1
                    assert b"not aligned" in L.ulcx_last_error()
            p, b = t(B, K, bs, ch, dtype=torch.float32), t(B, K, dtype=torch.int32)
            d_in = torch.from_numpy(np.ascontiguousarray(blocks[:, c * K:(c + 1) * K])).to(dev)
            dec.decode_dev(d_in.data_ptr(), wslot, K, p.data_ptr(), b.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(b.cpu().numpy(), wbits[:, c * K:(c + 1) * K]), f"decoder {i} call {c}: bits consumed differ"
            assert _same_bits(p.cpu().numpy(), want[:, c * K:(c + 1) * K]), f"decoder {i} call {c}: decoded samples differ"
    for dec in decs:
        dec.close()
    # byte streams need no alignment: odd slot / payload addresses are part of every guarded call above (carved at odd addresses)
