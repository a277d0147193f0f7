"""The window axis on the GPU: every WindowCtrl code the encoder's window control can emit, every form of the transform those
codes pick, and every boundary of a call's launch plan with a switched block on either side (tests/window_axis_testlib.py,
DESIGN.md "Window classes"), against the oracle alone, bit for bit - sizes, WindowCtrl, BlockComplexity bit patterns and
bytes, and through the debug taps coefficients, noise spectrum, keys, kept sets and nOutCoef (the comparison of
tests/test_gpu_parity.py); no tolerance anywhere, nothing timed.

tests/test_window_axis_capi.py asserts on the CPU what these streams reach: the full code set of every geometry, every block
class, every boundary.  The streams and the oracle's runs are computed once per process and shared."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd, to_dev
from ulc_testlib import to_pcm16
from test_gpu_parity import _compare_encode
import window_axis_testlib as W

pytestmark = pytest.mark.gpu

# the full table under the other call kinds at two geometries, and a third of it at each of the other eight (every third row of
# the table: every scale and, from 1024 on, every position), with the neighbour streams behind them everywhere
FULL_KINDS = [(2048, 2), (256, 2)]
THIRD_KINDS = [g for g in W.GEOMETRIES if g not in FULL_KINDS]
KIND_GEOS = pytest.mark.parametrize("geo", FULL_KINDS + THIRD_KINDS, ids=W.geo_id)


def _rows_of(geo):
    n = len(W.TABLE[geo])
    return list(range(n)) if geo in FULL_KINDS else list(range(0, n, 3))


def _pick(geo):
    """(pcm [n][10 * bs][ch], the oracle's runs) of the rows a geometry runs under the other kinds, the neighbour streams behind them."""
    bs, ch = geo
    rows = _rows_of(geo)
    pcm = np.concatenate([W.code_streams(bs, ch)[rows], W.neighbour_streams(bs, ch)])
    refs = [W.oracle_runs("code", bs, ch)[i] for i in rows] + list(W.oracle_runs("neighbour", bs, ch))
    return pcm, refs


def _open(n, geo, K):
    bs, ch = geo
    enc = _amd().BatchEncoder(n, ch, bs, W.RATE, K)
    assert enc.slot == 2 * ch * bs + 16
    return enc


def _encode_calls(enc, pcm, refs, bs, K, calls, what):
    """`calls` consecutive calls of K blocks, every stream and block against the oracle, taps included -> the blocks [n][calls * K][slot]."""
    outs = []
    for j in range(calls):
        res = enc.encode(pcm[:, j * K * bs:(j + 1) * K * bs])
        dbg = enc.debug_fetch(K)
        for s in range(pcm.shape[0]):
            _compare_encode(res, refs[s], s, j * K, K, dbg, f"{what} call {j}")
        outs.append(res[0])
    return np.concatenate(outs, axis=1)


# ---------------------------------------------------------------------------
# code cases: one stream per code of the table, two consecutive calls of 5 blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("geo", W.GEOMETRIES, ids=W.geo_id)
def test_every_code(geo):
    """One encoder per geometry, one stream per code (the switched block's index differs from stream to stream), and the streams
    with switched blocks in a row behind them."""
    bs, ch = geo
    pcm = np.concatenate([W.code_streams(bs, ch), W.neighbour_streams(bs, ch)])
    refs = list(W.oracle_runs("code", bs, ch)) + list(W.oracle_runs("neighbour", bs, ch))
    seen = {int(c) for r in refs for c in r["wc"]}
    assert seen == W.codes(bs) - set(W.NOT_REACHED.get(geo, ())), "the census (tests/test_window_axis_capi.py)"
    enc = _open(pcm.shape[0], geo, W.CODE_K)
    try:
        _encode_calls(enc, pcm, refs, bs, W.CODE_K, W.CODE_CALLS, f"{bs} x {ch} codes")
    finally:
        enc.close()


# ---------------------------------------------------------------------------
# the same streams under the other kinds
# ---------------------------------------------------------------------------
@KIND_GEOS
def test_pcm16_ingest(geo):
    """PCM16 ingest (blocks 0 and 1 of a call are never on the steady-state path; the streams lie on the PCM16 grid, so the
    oracle's run of the float samples is the reference)."""
    import torch
    bs, ch = geo
    pcm, refs = _pick(geo)
    n, K = pcm.shape[0], W.CODE_K
    enc = _open(n, geo, K)
    try:
        for j in range(W.CODE_CALLS):
            x = pcm[:, j * K * bs:(j + 1) * K * bs]
            x16 = to_pcm16(x)
            assert np.array_equal(x16.astype(np.float32) * np.float32(2.0 ** -15), x)
            d_in = to_dev(x16)
            d_out = torch.zeros((n, K, enc.slot), dtype=torch.uint8, device=d_in.device)
            d_bits, d_wc = (torch.zeros((n, K), dtype=torch.int32, device=d_in.device) for _ in range(2))
            d_cplx = torch.zeros((n, K), dtype=torch.float32, device=d_in.device)
            enc.encode_dev_pcm16(d_in.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), d_wc.data_ptr(), d_cplx.data_ptr())
            torch.cuda.synchronize()
            res = (d_out.cpu().numpy(), d_bits.cpu().numpy(), d_wc.cpu().numpy(), d_cplx.cpu().numpy())
            dbg = enc.debug_fetch(K)
            for s in range(n):
                _compare_encode(res, refs[s], s, j * K, K, dbg, f"{bs} x {ch} PCM16 call {j}")
    finally:
        enc.close()


@KIND_GEOS
def test_analysis_call(geo):
    """The analysis call (k_xfa, wc and cplx): WindowCtrl and BlockComplexity of every block, and through the clips form of the same
    call (ulcx_analyse_clips_host) the MDCT coefficients k_xfa leaves."""
    bs, ch = geo
    pcm, refs = _pick(geo)
    n, K = pcm.shape[0], W.CODE_K
    enc = _open(n, geo, K)
    try:
        for j in range(W.CODE_CALLS):
            wc, cplx = enc.analyse(pcm[:, j * K * bs:(j + 1) * K * bs])
            for s in range(n):
                for k in range(K):
                    kk = j * K + k
                    tag = f"{bs} x {ch} analyse stream {s} block {kk}"
                    assert wc[s, k] == refs[s]["wc"][kk], f"{tag}: WindowCtrl {wc[s, k]:#x} != {refs[s]['wc'][kk]:#x}"
                    assert cplx[s, k].tobytes() == refs[s]["cplx"][kk].tobytes(), f"{tag}: BlockComplexity {cplx[s, k]!r} != {refs[s]['cplx'][kk]!r}"
        # The same transform with its coefficients tapped: the streams as clips (from a fresh state, in chunks of maxBlocksPerCall
        # = 5 blocks: the two calls above).  BlockComplexity alone does not see every coefficient - on a noise bed it sits at its
        # upper clamp 1.0 for two channels and more.
        coef, cwc, ccplx = enc.analyse_clips(np.ascontiguousarray(pcm.transpose(0, 2, 1)), n_blocks=W.CODE_BLOCKS)
        for s in range(n):
            want = refs[s]["coef"].reshape(W.CODE_BLOCKS, ch, bs).transpose(1, 0, 2)
            assert np.array_equal(cwc[s], refs[s]["wc"]) and ccplx[s].tobytes() == refs[s]["cplx"].tobytes(), f"{bs} x {ch} analyse_clips stream {s}: wc / cplx"
            diff = np.ascontiguousarray(coef[s]).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
            if diff.any():
                c, k, i = (int(v) for v in np.argwhere(diff)[0])
                raise AssertionError(f"{bs} x {ch} analyse_clips stream {s} block {k} (WindowCtrl {refs[s]['wc'][k]:#x}) channel {c}: MDCT coefficients differ "
                                     f"from line {i} ({int(diff[:, k].sum())} in the block)")
    finally:
        enc.close()


@KIND_GEOS
def test_decoder_on_the_encoders_bytes(geo):
    """The encoder's own bytes through BatchDecoder against the oracle's decode of the oracle's bytes, PCM bit for bit: every
    emitted code with real neighbours rather than hand-assembled ones."""
    bs, ch = geo
    pcm, refs = _pick(geo)
    n, K = pcm.shape[0], W.CODE_K
    _, want_code, bits_code = W.oracle_decoded("code", bs, ch)
    _, want_nb, bits_nb = W.oracle_decoded("neighbour", bs, ch)
    want = np.concatenate([want_code[_rows_of(geo)], want_nb])
    want_bits = np.concatenate([bits_code[_rows_of(geo)], bits_nb])
    enc = _open(n, geo, K)
    dec = _amd().BatchDecoder(n, ch, bs, K)
    try:
        blocks = _encode_calls(enc, pcm, refs, bs, K, W.CODE_CALLS, f"{bs} x {ch} encode for the decoder")
        for j in range(W.CODE_CALLS):
            got, gbits = dec.decode(blocks[:, j * K:(j + 1) * K])
            assert np.array_equal(gbits, want_bits[:, j * K:(j + 1) * K]), f"{bs} x {ch} decode call {j}: sizes consumed"
            w = want[:, j * K * bs:(j + 1) * K * bs]
            diff = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
            if diff.any():
                s, t, c = (int(v) for v in np.argwhere(diff)[0])
                raise AssertionError(f"{bs} x {ch} decode: stream {s} block {j * K + t // bs} (WindowCtrl {refs[s]['wc'][j * K + t // bs]:#x}): PCM differs from "
                                     f"sample {t % bs} channel {c}: {got[s, t, c]!r} != {w[s, t, c]!r} ({int(diff.sum())} samples differ)")
    finally:
        enc.close(); dec.close()


@KIND_GEOS
def test_clips_cut_at_the_switched_block(geo):
    """The clips call with maxBlocksPerCall cutting a clip directly in front of and directly behind its switched block: the code
    streams grouped by the block j their event switches, on an object of maxBlocksPerCall = j (a chunk ends in front of block j)
    and on one of j + 1 (a chunk ends behind it).  Payload bytes, sizes, block counts and index rows against the oracle's run
    of the clip alone."""
    from clips_testlib import ClipRef, SCALAR
    bs, ch = geo
    rows = _rows_of(geo)
    pcm = W.code_streams(bs, ch)
    amd = _amd()
    groups = {}
    for i in rows:
        wc = W.oracle_runs("code", bs, ch)[i]["wc"]
        e = W.code_event_block(*W.TABLE[geo][i][1:])
        groups.setdefault(e + 1 if W.switched(int(wc[e + 1])) else e + 2, []).append(i)      # the first block the event switches
    for j, members in sorted(groups.items()):
        wave = np.ascontiguousarray(pcm[members].transpose(0, 2, 1))
        refs = [ClipRef(bs, ch, w, SCALAR) for w in wave]
        for i, r in zip(members, refs):
            assert W.switched(int(r.wc[j])), f"{bs} x {ch} stream {i}: block {j} is not switched"
        for M in (j, j + 1):
            enc = amd.BatchEncoder(len(members), ch, bs, W.RATE, M)
            dec = amd.BatchDecoder(len(members), ch, bs, refs[0].nb + 1)
            try:
                payload, nbytes, maxb, index, count = enc.encode_clips(dec, wave)
                for k, (i, r) in enumerate(zip(members, refs)):
                    where = f"{bs} x {ch} clips, maxBlocksPerCall {M}, stream {i} (switched block {j})"
                    total = int(r.sizes.sum())
                    assert count[k] == r.nb and nbytes[k] == total and maxb[k] == int(r.sizes.max()), f"{where}: {count[k]} blocks, {nbytes[k]} bytes"
                    if not np.array_equal(payload[k, :total], r.payload):
                        bad = int(np.argmax(payload[k, :total] != r.payload))
                        edges = np.concatenate([[0], np.cumsum(r.sizes)])
                        raise AssertionError(f"{where}: payload differs from byte {bad} (block {int(np.searchsorted(edges, bad, 'right')) - 1})")
                    assert index[k].tobytes() == r.index_row(index.shape[1]).tobytes(), f"{where}: index row"
            finally:
                enc.close(); dec.close()


# ---------------------------------------------------------------------------
# position cases: a switched block on either side of every boundary of the launch plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", W.POSITION_KS)
@pytest.mark.parametrize("geo", W.POSITION_GEOMETRIES, ids=W.geo_id)
def test_switched_blocks_at_every_boundary(geo, K):
    """Two calls of K blocks; the call's steps and cuts as the library reports them (ulcx_encoder_debug_front_plan: the function
    the launch calls) against the model.  On an object without side streams every K takes the plain plan: the test says so and
    still compares."""
    bs, ch = geo
    pcm = W.position_streams(bs, ch, K)
    refs = W.oracle_runs("position", bs, ch, K)
    enc = _open(pcm.shape[0], geo, K)
    try:
        pipe = enc.plan()["wc_pipe"]
        assert pipe in (1, W.WC_PIPE), f"wc_pipe = {pipe}"
        if pipe == 1:
            print(f"{bs} x {ch} K = {K}: this object has no side streams - the plain plan for every K")
        for k in sorted({K, 1, 5, 6, 7, 8}):
            if k <= K:
                assert enc.front_plan(k) == W.front_plan(k, pipe), f"{bs} x {ch}: front plan of {k} blocks {enc.front_plan(k)}, the model {W.front_plan(k, pipe)}"
        for k in (0, K + 1):
            with pytest.raises(_amd().UlcError, match="ulcx_encoder_debug_front_plan: nBlocks out of range"):
                enc.front_plan(k)
        _encode_calls(enc, pcm, refs, bs, K, 2, f"{bs} x {ch} K = {K} cuts {enc.front_plan(K)[0]} steps {enc.front_plan(K)[1]}")
    finally:
        enc.close()
