"""The sample-rate axis on the GPU: every Bark ring class (tests/rate_axis_testlib.py, DESIGN.md "Ring classes") on every
encoder path, bit-exact against the oracle - sizes, WindowCtrl, BlockComplexity bit patterns and bytes, no tolerance anywhere.

Each case opens one encoder and asserts from ulcx_encoder_debug_plan that the object is in the class the case is named for
(tests/test_band_plan_capi.py asserts the same from the band tables alone, on the CPU: a case cannot pass on the wrong path).
A batch is 70 streams - 840 noise rows in stereo, 13 full tiles of k_bark_uniform and a tail of 8 - tiled from 5 distinct
streams in a seeded permutation, two calls of 6 blocks, so state carries and the window-control pipeline has chunks; every
copy is compared with its distinct stream's oracle encode."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd
import rate_axis_testlib as R

pytestmark = pytest.mark.gpu


def _open(bs, ch, rate, cls, B, K, fields=None):
    """An encoder, with its plan checked against the class of the case."""
    enc = _amd().BatchEncoder(B, ch, bs, rate, K)
    plan = enc.plan()
    try:
        assert R.in_class(plan["most_open"], plan["bark_ring"], cls), f"{bs} x {ch} at {rate} Hz: {plan}, the case wants (ring, most) = {cls}"
        for k, v in (fields or {}).items():
            assert plan[k] == v, f"{bs} x {ch} at {rate} Hz: plan {k} = {plan[k]}, the case wants {v}"
    except BaseException:
        enc.close()
        raise
    return enc, plan


def _both_kinds(refs):
    """Among the blocks that keep coefficients there are decimated and un-decimated ones: on a ring either kind takes its own
    Bark kernels, and the levels of a block that keeps nothing decide little."""
    dec = np.concatenate([R.decimated(r["wc"])[r["nout"] > 0] for r in refs])
    assert dec.any() and not dec.all(), f"{int(dec.sum())} of {dec.size} blocks with kept coefficients are decimated"


def _batch(bs, ch, rate, cls, mode, B=70, K=6, calls=2, sel_pair=None):
    distinct = R.distinct_streams(bs, ch, rate, calls * K, seed=bs + rate)
    pcm, src = R.tiled(distinct, B, seed=bs + ch)
    enc, plan = _open(bs, ch, rate, cls, B, K, None if sel_pair is None else dict(sel_pair=sel_pair))
    try:
        refs = R.oracle_refs(distinct, bs, rate, mode, enc.slot)
        _both_kinds(refs)
        for c in range(calls):
            res = enc.encode(pcm[:, c * K * bs:(c + 1) * K * bs], *mode)
            R.compare_call(res, refs, src, c * K, f"{bs} x {ch} at {rate} Hz mode {mode} call {c}")
    finally:
        enc.close()


@pytest.mark.parametrize("case", R.BATCH_CASES, ids=R.case_id)
def test_batch_vbr_bit_exact_in_every_ring_class(case):
    bs, ch, rate, cls = case
    _batch(bs, ch, rate, cls, R.VBR50, sel_pair=1 if (bs, ch) == (4096, 2) else 0)


@pytest.mark.parametrize("case", R.MODE_CASES, ids=R.case_id)
def test_batch_rate_search_bit_exact_off_ring_4(case):
    """CBR / ABR: the probes of the rate search read the noise and masking levels of ring 0 and ring 8 objects."""
    bs, ch, rate, cls, mode = case
    _batch(bs, ch, rate, cls, mode)


@pytest.mark.parametrize("case", R.BIG_CASES, ids=R.case_id)
def test_big_blocks_bit_exact(case):
    """One call of 3 blocks, 3 streams, no tiling: white noise (its third block is un-decimated), last channel silent, an impulse
    in every block.  A stream's first block keeps no coefficient, so three blocks are the fewest.  The two cases that
    name where the exact path's heap lives (16384 coefficients: the largest heap LDS takes; 24576: the object's scratch) then run
    the same call from a fresh state with every block handed to that path: the same bytes, and the path's count says it ran."""
    bs, ch, rate, cls, fields = case
    B = K = 3
    distinct = R.distinct_streams(bs, ch, rate, K, seed=bs + rate)[[2, 3, R.IMPULSE]]
    src = np.arange(B)
    enc, plan = _open(bs, ch, rate, cls, B, K, fields)
    try:
        refs = R.oracle_refs(distinct, bs, rate, R.VBR50, enc.slot)
        _both_kinds(refs)
        res = enc.encode(distinct, *R.VBR50)
        R.compare_call(res, refs, src, 0, f"{bs} x {ch} at {rate} Hz")
        if "heap_in_lds" in fields:
            enc.reset()
            enc.force_exact(1)
            res = enc.encode(distinct, *R.VBR50)
            assert enc.last_fallbacks() == sum(int((r["nout"] > 0).sum()) for r in refs) >= 2 * B      # (a block that keeps nothing has no cut)
            R.compare_call(res, refs, src, 0, f"{bs} x {ch} at {rate} Hz, every block on the exact path")
    finally:
        enc.close()


@pytest.mark.parametrize("case", R.TILE_CASES, ids=R.case_id)
def test_whole_tiles_of_decimated_rows(case):
    """Streams 32..63 of 100 are the impulse-per-block stream, 4 blocks a call: blocks 128..255 of a call are noise rows 256..511,
    four whole tiles of k_bark_uniform, and masking rows 128..255, two whole tiles.  A stream's very first block is never
    decimated (window control starts from a full-size window), so the first call leaves 16 rows of each of those tiles
    un-decimated; in the SECOND call every block of these streams is decimated and no row of those tiles is the kernel's - the
    workgroup leaves at its first ballot, and k_nbark / k_pbark take the rows from the transform's list (128 entries).  Ordinary
    streams on both sides.  Asserted from the oracle's window codes: every block of the impulse stream behind the first is
    decimated, and the second call has at least one whole tile of noise rows and one of masking rows without an un-decimated
    row."""
    bs, ch, rate, cls = case
    B, K, calls = 100, 4, 2
    distinct = R.distinct_streams(bs, ch, rate, calls * K, seed=bs + rate)
    others = np.array([i for i in range(len(distinct)) if i != R.IMPULSE])
    src = others[np.random.default_rng([0x7115, rate]).integers(0, len(others), B)]
    src[32:64] = R.IMPULSE
    pcm = distinct[src]
    enc, plan = _open(bs, ch, rate, cls, B, K)
    try:
        refs = R.oracle_refs(distinct, bs, rate, R.VBR50, enc.slot)
        dec = np.stack([R.decimated(refs[i]["wc"]) for i in src])                       # [B][calls * K]
        assert dec[32:64, 1:].all(), f"the impulse stream's window codes {[hex(w) for w in refs[R.IMPULSE]['wc']]}: a block behind the first is not decimated"
        assert not dec[:32].all(axis=1).any() and not dec[64:].all(axis=1).any(), "an ordinary stream without an un-decimated block"
        masking_rows = dec[:, K:2 * K].reshape(-1)                                      # row = stream * K + block of the call
        noise_rows = np.repeat(masking_rows, ch)                                        # row = (stream * K + block) * channels + channel
        for rows, what in ((noise_rows, "noise"), (masking_rows, "masking")):
            full = rows[:rows.size // 64 * 64].reshape(-1, 64).all(axis=1)
            assert full.any() and not full.all(), f"second call: no whole tile of decimated {what} rows (or nothing else)"
        for c in range(calls):
            res = enc.encode(pcm[:, c * K * bs:(c + 1) * K * bs], *R.VBR50)
            R.compare_call(res, refs, src, c * K, f"{bs} x {ch} at {rate} Hz tiles, call {c}")
    finally:
        enc.close()


def test_two_encoders_of_different_rings_interleaved():
    """Ring 0 and ring 4 objects alive on one device, their calls alternating: the dynamic-LDS allowance is per kernel, the
    table blobs and the decimated-block lists per object.  Each equals its own oracle."""
    B, K, calls = 6, 6, 2
    encs = []
    try:
        for bs, ch, rate, cls in R.PAIR_CASES:
            distinct = R.distinct_streams(bs, ch, rate, calls * K, seed=bs + rate)
            pcm, src = R.tiled(distinct, B, seed=rate)
            enc, plan = _open(bs, ch, rate, cls, B, K)
            encs.append((enc, pcm, src, R.oracle_refs(distinct, bs, rate, R.VBR50, enc.slot), bs, rate))
        assert encs[0][0].plan()["bark_ring"] != encs[1][0].plan()["bark_ring"]
        for c in range(calls):
            got = [enc.encode(pcm[:, c * K * bs:(c + 1) * K * bs], *R.VBR50) for enc, pcm, src, refs, bs, rate in encs]
            for res, (enc, pcm, src, refs, bs, rate) in zip(got, encs):
                R.compare_call(res, refs, src, c * K, f"interleaved, {rate} Hz, call {c}")
    finally:
        for e in encs:
            e[0].close()
