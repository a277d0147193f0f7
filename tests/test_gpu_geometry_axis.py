"""The geometry axis on the GPU: every selection, transform, window-control, gap-sum and heap class (tests/geometry_axis_testlib.py,
DESIGN.md "Geometry classes") under every call kind that reaches it, against the oracle alone - sizes, WindowCtrl,
BlockComplexity bit patterns, bytes and, where debug_fetch gives them, kept sets and nOutCoef; no tolerance anywhere.

Every object asserts from ulcx_encoder_debug_plan that the library put it where the model says (gap sums, heap in LDS, pair
selection); tests/test_geometry_axis_capi.py asserts on the CPU that the cases fill the classes and that the oracle's runs hold
live decimated and un-decimated blocks, silent blocks, and starved and saturated rate searches.  A case is 7 streams in two calls
of 3 and 6 blocks on one object; the oracle's runs are computed once per process and shared."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd, to_dev
from ulc_testlib import to_pcm16
import geometry_axis_testlib as G

pytestmark = pytest.mark.gpu


def _cases(kind):
    return pytest.mark.parametrize("case", G.cases_of(kind), ids=G.case_id)


def _open(bs, ch):
    """An encoder of the case, its plan checked against the model."""
    enc = _amd().BatchEncoder(G.B, ch, bs, G.RATE, G.KMAX)
    try:
        plan = enc.plan()
        for k, v in G.plan_fields(bs, ch).items():
            assert plan[k] == v, f"{bs} x {ch}: plan {k} = {plan[k]}, the model {G.classes(bs, ch)} wants {v}"
    except BaseException:
        enc.close()
        raise
    return enc


def _calls(bs, ch):
    """(call, first block, blocks, the call's samples [B][K * bs][ch])"""
    pcm = G.streams(bs, ch)
    return [(j, k0, K, pcm[:, k0 * bs:(k0 + K) * bs]) for j, k0, K in G.call_spans()]


def _taps(enc, K):
    return enc.debug_fetch(K, parts=("keep", "nout"))


def _scalar_calls(bs, ch, setting, what, force=0):
    """Both calls under one scalar setting on a fresh object -> the exact path's block count over both calls."""
    refs = G.oracle_rows(bs, ch, setting)
    enc = _open(bs, ch)
    fallbacks = 0
    try:
        if force:
            enc.force_exact(force)
        for j, k0, K, x in _calls(bs, ch):
            res = enc.encode(x, *G.scalar(setting))
            taps = _taps(enc, K)
            if force:
                n = enc.last_fallbacks()
                assert n > 0, f"{bs} x {ch} {what} call {j}: no block took the exact path"
                fallbacks += n
            G.compare_call(res, refs, j, k0, f"{bs} x {ch} {what}", taps, bs)
    finally:
        enc.close()
    return fallbacks


@_cases("vbr")
def test_vbr(case):
    """Scalar VBR 50: the one-pass selection (PASS 0)."""
    _scalar_calls(*case, G.VBR50, "VBR 50")


@_cases("search")
def test_search(case):
    """Scalar CBR at 48 kbps per channel pair and ABR (96, 0.45) on a second object: the probes of the rate search (PASS 1 / 2) and
    k_rate_step."""
    bs, ch = case
    _scalar_calls(bs, ch, G.cbr_of(ch), f"CBR {G.cbr_of(ch)[0]:g}")
    _scalar_calls(bs, ch, G.ABR96, "ABR (96, 0.45)")


@_cases("table")
def test_table(case):
    """encode_rates with a setting per stream: VBR 1 / 50 / 100, CBR 32 and 48 per channel pair, ABR (64, 0.2) and (128, 0.5) - the
    *_rates selection kernels, searching and one-pass blocks side by side."""
    bs, ch = case
    table = G.table_of(ch)
    refs = G.oracle_rows(bs, ch, table)
    enc = _open(bs, ch)
    try:
        for j, k0, K, x in _calls(bs, ch):
            res = enc.encode_rates(x, np.array(table, np.float32))
            G.compare_call(res, refs, j, k0, f"{bs} x {ch} table", _taps(enc, K), bs)
    finally:
        enc.close()


@_cases("ladder")
def test_ladder(case):
    """Three rungs (VBR 50, CBR, VBR 100) in one call: every rung against its own oracle run; the taps are the last rung's."""
    bs, ch = case
    rungs = G.ladder_of(ch)
    refs = [G.oracle_rows(bs, ch, g) for g in rungs]
    enc = _open(bs, ch)
    try:
        for j, k0, K, x in _calls(bs, ch):
            out, bits, wc, cplx = enc.encode_ladder(x, [G.scalar(g) for g in rungs])
            assert out.shape == (len(rungs), G.B, K, enc.slot) and enc.last_rungs() == len(rungs)
            taps = _taps(enc, K)
            for r in range(len(rungs)):
                G.compare_call((out[r], bits[r], wc, cplx), refs[r], j, k0, f"{bs} x {ch} ladder rung {r} {rungs[r]}", taps if r == len(rungs) - 1 else None, bs)
    finally:
        enc.close()


@_cases("exact")
def test_exact(case):
    """force_exact(2): every second block through the exact (heapsort-rank) path, heap in LDS or in the object's scratch, with
    and without gap sums; VBR, CBR and ABR."""
    bs, ch = case
    counts = [_scalar_calls(bs, ch, setting, f"exact {setting}", force=2) for setting in (G.VBR50, G.cbr_of(ch), G.ABR96)]
    print(f"{bs} x {ch} {G.classes(bs, ch)}: blocks on the exact path under VBR 50 / CBR / ABR: {counts}")


@_cases("analyse")
def test_analyse(case):
    """The analysis call (k_xfa*, k_cplxa) of every transform and window-control class: WindowCtrl and BlockComplexity."""
    bs, ch = case
    refs = G.oracle_rows(bs, ch, G.VBR50)
    enc = _open(bs, ch)
    try:
        for j, k0, K, x in _calls(bs, ch):
            wc, cplx = enc.analyse(x)
            G.compare_series(wc, cplx, refs, j, k0, f"{bs} x {ch} analyse")
    finally:
        enc.close()


@_cases("pcm16")
def test_pcm16(case):
    """PCM16 ingest of every transform and window-control class: the per-stream-table call (one-pass and searching blocks) and the
    analysis call.  The streams lie on the PCM16 grid, so the oracle's run of the float samples is the reference: equal to it is
    equal to float ingest (test_table, test_analyse)."""
    import torch
    bs, ch = case
    table = G.table_of(ch)
    refs = G.oracle_rows(bs, ch, table)
    enc, ana = _open(bs, ch), _open(bs, ch)
    try:
        for j, k0, K, x in _calls(bs, ch):
            x16 = to_pcm16(x)
            assert np.array_equal(x16.astype(np.float32) * np.float32(2.0 ** -15), x)
            d_in = to_dev(x16)
            d_out = torch.zeros((G.B, K, enc.slot), dtype=torch.uint8, device=d_in.device)
            d_bits, d_wc = (torch.zeros((G.B, K), dtype=torch.int32, device=d_in.device) for _ in range(2))
            d_cplx = torch.zeros((G.B, K), dtype=torch.float32, device=d_in.device)
            d_rates = to_dev(np.array(table, np.float32))
            enc.encode_dev_rates(d_rates.data_ptr(), d_in.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), d_wc.data_ptr(), d_cplx.data_ptr(), pcm16=True)
            torch.cuda.synchronize()
            res = (d_out.cpu().numpy(), d_bits.cpu().numpy(), d_wc.cpu().numpy(), d_cplx.cpu().numpy())
            G.compare_call(res, refs, j, k0, f"{bs} x {ch} PCM16 encode", _taps(enc, K), bs)
            a_wc = torch.zeros((G.B, K), dtype=torch.int32, device=d_in.device)
            a_cplx = torch.zeros((G.B, K), dtype=torch.float32, device=d_in.device)
            ana.analyse_dev(d_in.data_ptr(), K, a_wc.data_ptr(), a_cplx.data_ptr(), pcm16=True)
            torch.cuda.synchronize()
            G.compare_series(a_wc.cpu().numpy(), a_cplx.cpu().numpy(), refs, j, k0, f"{bs} x {ch} PCM16 analyse")
    finally:
        enc.close(); ana.close()


@_cases("decode")
def test_decode(case):
    """The oracle's VBR 50 streams through BatchDecoder, in calls of 3 and 6 blocks: PCM and consumed sizes equal to the oracle's own
    decode, bit for bit (k_dgen at 1 to 255 channels, k_dsyn at every size).  Every geometry here must open."""
    bs, ch = case
    blocks, pcm, bits = G.oracle_decoded(bs, ch)
    dec = _amd().BatchDecoder(G.B, ch, bs, G.KMAX)
    try:
        for j, k0, K in G.call_spans():
            got, gbits = dec.decode(blocks[:, k0:k0 + K])
            want = pcm[:, k0 * bs:(k0 + K) * bs]
            bad = np.argwhere(gbits != bits[:, k0:k0 + K])
            assert bad.size == 0, f"{bs} x {ch} decode: stream {bad[0][0]} call {j} block {bad[0][1]}: {gbits[tuple(bad[0])]} bits consumed, the oracle {bits[bad[0][0], k0 + bad[0][1]]}"
            diff = np.ascontiguousarray(got).view(np.uint32) != want.view(np.uint32)
            if diff.any():
                s, n, c = (int(v) for v in np.argwhere(diff)[0])
                raise AssertionError(f"{bs} x {ch} decode: stream {s} call {j} block {n // bs} (block {k0 + n // bs} of the stream): PCM differs from sample "
                                     f"{n % bs} channel {c}: {got[s, n, c]!r} != {want[s, n, c]!r} ({int(diff.sum())} samples differ)")
    finally:
        dec.close()
