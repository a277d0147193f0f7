"""Ladder calls (include/ulc_amd.h ulcx_encode_*_ladder, ulcx-tool RATE = R0/R1/...): several rate settings per stream in
one call.  Every rung must be what an encoder of its own writes under that rung's setting - checked against the oracle
(one orc_encoder per stream and rung, tests/rates_testlib.py), never against the library itself - and, second, what the
plain / per-stream-rates calls give on separate encoders; the streams' state advances once per call."""
import functools
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from ulc_testlib import write_wav16, run_tool
from gpu_testlib import amd as _ulc
from ulc_testlib import synth_pcm, oracle_encode_debug
from rates_testlib import oracle_streams

pytestmark = pytest.mark.gpu

VBR, CBR, ABR = 0, 1, 2
# six entries of MIXED (tests/test_gpu_stream_rates.py): CBR 32, ABR (64, 0.02), VBR 37.5, ABR (64, 0.35), VBR 100, ABR (128, 0.98)
TABLE6 = [(32.0, 0.0), (64.0, 0.02), (-37.5, 0.0), (64.0, 0.35), (-100.0, 0.0), (128.0, 0.98)]
FIVE = [(VBR, 50.0, 0.0), (CBR, 64.0, 0.0), TABLE6, (VBR, 100.0, 0.0), (ABR, 96.0, 0.3)]


def _batch_pcm(B, n, ch, rate, seed):
    return np.stack([synth_pcm(s, n, ch, rate, transient=(s % 3 != 1), seed=seed) for s in range(B)])


def _settings(rung, B):
    """A rung as the per-stream settings [B] of the tool's convention (what the oracle driver takes)."""
    if isinstance(rung, tuple):
        mode, p0, p1 = rung
        return [(-p0, 0.0) if mode == VBR else (p0, p1 if mode == ABR else 0.0)] * B
    assert len(rung) == B
    return list(rung)


def _lib_rung(rung):
    return rung if isinstance(rung, tuple) else np.array(rung, np.float32)


def _oracle_ladder(pcm, bs, rate, rungs, calls):
    """ref[r][s][block]: one oracle encoder per stream and rung, the rung's setting constant over all calls."""
    B = pcm.shape[0]
    return [oracle_streams(pcm, bs, rate, [_settings(g, B)] * calls) for g in rungs]


def _check_call(j, K, res, ref, what, taps=None):
    out, bits, wc, cplx = res
    R, B = out.shape[0], out.shape[1]
    for r in range(R):
        for s in range(B):
            for k in range(K):
                o = ref[r][s][j * K + k]
                tag = f"{what}: rung {r} stream {s} call {j} block {k}"
                assert bits[r, s, k] == o["bits"], f"{tag}: bits {bits[r, s, k]} != oracle {o['bits']}"
                assert np.array_equal(out[r, s, k, :bits[r, s, k] // 8], o["bytes"]), f"{tag}: bytes differ"
                if r == 0:
                    assert wc[s, k] == o["wc"], f"{tag}: WindowCtrl"
                    assert cplx[s, k].view(np.uint32) == o["cplx"].view(np.uint32), f"{tag}: BlockComplexity"
                if taps is not None and r == R - 1:
                    assert taps["nout"][s, k] == o["nout"], f"{tag}: nOutCoef {taps['nout'][s, k]} != {o['nout']}"
                    assert np.array_equal(taps["keep"][s, k], o["keep"]), f"{tag}: kept set differs"


def _same_blocks(ao, ab, bo, bb, what):
    assert np.array_equal(ab, bb), f"{what}: sizes differ"
    for idx in np.ndindex(ab.shape):
        assert np.array_equal(ao[idx][:ab[idx] // 8], bo[idx][:bb[idx] // 8]), f"{what}: bytes differ at {idx}"


@functools.lru_cache(maxsize=None)
def _five_rung_case():
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 6
    pcm = _batch_pcm(B, 2 * K * bs, ch, rate, seed=41)
    pcm.setflags(write=False)
    return pcm, _oracle_ladder(pcm, bs, rate, FIVE, 2)


@pytest.mark.parametrize("force", [0, 2])
def test_five_rungs_are_bit_exact_per_rung(force):
    """Stereo BlockSize 2048 at 44.1 kHz, six streams, K = 4, two consecutive ladder calls of five rungs (scalar VBR, scalar
    CBR, a mixed per-stream table, scalar VBR 100, scalar ABR); force = 2 sends every second block of every rung through
    the exact (heapsort-rank) path."""
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 6
    pcm, ref = _five_rung_case()
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    if force:
        enc.force_exact(force)
    for j in range(2):
        res = enc.encode_ladder(pcm[:, j * K * bs:(j + 1) * K * bs], [_lib_rung(g) for g in FIVE])
        assert res[0].shape == (5, B, K, enc.slot) and res[1].shape == (5, B, K)
        taps = enc.debug_fetch(K, parts=("keep", "nout"))
        if force:
            assert enc.last_fallbacks() > 0
        _check_call(j, K, res, ref, f"five rungs (force_exact {force})", taps)
    assert enc.last_rungs() == 5
    enc.close()


def test_a_rung_does_not_depend_on_its_position_or_neighbours():
    """The five rungs rotated give rung for rung the same blocks; one rung alone equals the plain call and the per-stream-rates
    call with a uniform table; last_rungs() follows the calls."""
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 6
    pcm, _ = _five_rung_case()
    x = pcm[:, :K * bs]
    a = ulc.BatchEncoder(B, ch, bs, rate, K)
    ao, ab, aw, ac = a.encode_ladder(x, [_lib_rung(g) for g in FIVE])
    assert a.last_rungs() == 5
    for shift in (1, 3):
        order = [(r + shift) % 5 for r in range(5)]
        b = ulc.BatchEncoder(B, ch, bs, rate, K)
        bo, bb, bw, bc = b.encode_ladder(x, [_lib_rung(FIVE[r]) for r in order])
        assert np.array_equal(aw, bw) and np.array_equal(ac.view(np.uint32), bc.view(np.uint32))
        for pos, r in enumerate(order):
            _same_blocks(ao[r], ab[r], bo[pos], bb[pos], f"rung {r} at position {pos}")
        b.close()
    # one rung: the plain call, and the per-stream-rates call with a uniform table
    for r, (mode, p0, p1) in ((0, FIVE[0]), (1, FIVE[1]), (4, FIVE[4])):
        one, plain, tab = (ulc.BatchEncoder(B, ch, bs, rate, K) for _ in range(3))
        oo, ob, ow, oc = one.encode_ladder(x, [(mode, p0, p1)])
        assert one.last_rungs() == 1 and oo.shape[0] == 1
        po, pb, pw, pc = plain.encode(x, mode, p0, p1)
        assert plain.last_rungs() == 1
        to, tb, tw, tc = tab.encode_rates(x, np.array(_settings(FIVE[r], B), np.float32))
        assert tab.last_rungs() == 1
        _same_blocks(oo[0], ob[0], po, pb, f"one-rung ladder vs plain call, rung {r}")
        _same_blocks(oo[0], ob[0], to, tb, f"one-rung ladder vs uniform table, rung {r}")
        _same_blocks(ao[r], ab[r], po, pb, f"rung {r} of five vs plain call")
        assert np.array_equal(ow, pw) and np.array_equal(oc.view(np.uint32), pc.view(np.uint32))
        for e in (one, plain, tab):
            e.close()
    a.analyse(x)
    assert a.last_rungs() == 0
    a.close()


@pytest.mark.parametrize("first", ["ladder", "analyse"])
def test_state_advances_once(first):
    """A ladder call (or an analysis call), then a plain VBR call on the next K blocks: the same blocks as the second of two
    plain VBR calls."""
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 6
    pcm, _ = _five_rung_case()
    x0, x1 = pcm[:, :K * bs], pcm[:, K * bs:2 * K * bs]
    a = ulc.BatchEncoder(B, ch, bs, rate, K)
    b = ulc.BatchEncoder(B, ch, bs, rate, K)
    if first == "ladder":
        a.encode_ladder(x0, [_lib_rung(g) for g in FIVE])
    else:
        a.analyse(x0)
    b.encode(x0, VBR, 50.0)
    ao, ab, aw, ac = a.encode(x1, VBR, 50.0)
    bo, bb, bw, bc = b.encode(x1, VBR, 50.0)
    assert np.array_equal(aw, bw) and np.array_equal(ac.view(np.uint32), bc.view(np.uint32))
    _same_blocks(ao, ab, bo, bb, f"plain call behind a {first} call")
    a.close(); b.close()


@pytest.mark.parametrize("ch,bs,rate,transient", [(1, 256, 44100, True), (2, 4096, 48000, True), (6, 1024, 44100, False)])
def test_other_geometries(ch, bs, rate, transient):
    """Mono 256; stereo 4096 at 48 kHz with window switching (k_select_pair, decimated blocks); six channels x 1024 (the
    generic k_select on keys finalised once per call).  Three rungs, two calls, against the oracle."""
    ulc = _ulc()
    K, B = 3, 5
    rungs = [(VBR, 50.0, 0.0), (CBR, 48.0, 0.0), [(-90.0, 0.0), (128.0, 0.5), (32.0, 0.0), (-20.0, 0.0), (64.0, 0.2)]]
    pcm = np.stack([synth_pcm(s, 2 * K * bs, ch, rate, transient=transient, seed=44) for s in range(B)])
    ref = _oracle_ladder(pcm, bs, rate, rungs, 2)
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    for j in range(2):
        res = enc.encode_ladder(pcm[:, j * K * bs:(j + 1) * K * bs], [_lib_rung(g) for g in rungs])
        taps = enc.debug_fetch(K, parts=("keep", "nout"))
        _check_call(j, K, res, ref, f"{ch}ch BlockSize {bs}", taps)
    enc.close()


def test_device_form_with_pcm16_ingest_equals_the_float_ladder():
    import torch
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 6
    pcm = _batch_pcm(B, K * bs, ch, rate, seed=45)
    pcm16 = np.clip(np.rint(pcm * 32768.0), -32768, 32767).astype(np.int16)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    d_table = torch.tensor(TABLE6, dtype=torch.float32, device=dev)
    rungs = [g if isinstance(g, tuple) else d_table.data_ptr() for g in FIVE]
    R = len(rungs)
    outs = []
    for use16 in (False, True):
        enc = ulc.BatchEncoder(B, ch, bs, rate, K)
        d_in = torch.from_numpy(pcm16).to(dev) if use16 else torch.from_numpy(pcm16.astype(np.float32) * np.float32(2.0 ** -15)).to(dev)
        d_out = torch.zeros((R, B, K, enc.slot), dtype=torch.uint8, device=dev)
        d_bits = torch.zeros((R, B, K), dtype=torch.int32, device=dev)
        d_cplx = torch.zeros((B, K), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        enc.encode_dev_ladder(rungs, d_in.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), 0, d_cplx.data_ptr(),
                              stream=st.cuda_stream, pcm16=use16)
        st.synchronize()
        assert enc.last_rungs() == R
        outs.append((d_out.cpu().numpy(), d_bits.cpu().numpy(), d_cplx.cpu().numpy()))
        enc.close()
    assert (outs[0][1] > 0).all()
    _same_blocks(outs[0][0], outs[0][1], outs[1][0], outs[1][1], "PCM16 ingest vs float")
    assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32))
    # ... and the host form on the same samples
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    ho, hb, hw, hc = enc.encode_ladder(pcm16.astype(np.float32) * np.float32(2.0 ** -15), [_lib_rung(g) for g in FIVE])
    _same_blocks(outs[0][0], outs[0][1], ho, hb, "device form vs host form")
    enc.close()


def test_validation_on_a_live_encoder_leaves_its_state_untouched():
    ulc = _ulc()
    bs, ch, rate, K, B = 1024, 2, 44100, 2, 4
    good_table = np.array([(-50.0, 0.0), (64.0, 0.0), (96.0, 0.3), (-70.0, 0.0)], np.float32)
    good = [(VBR, 50.0, 0.0), good_table, (CBR, 64.0, 0.0)]
    pcm = _batch_pcm(B, 3 * K * bs, ch, rate, seed=47)
    a = ulc.BatchEncoder(B, ch, bs, rate, K)
    b = ulc.BatchEncoder(B, ch, bs, rate, K)
    x0, x1, x2 = (pcm[:, j * K * bs:(j + 1) * K * bs] for j in range(3))
    a.encode_ladder(x0, good); b.encode_ladder(x0, good)
    refused = [[], [(VBR, 50.0, 0.0)] * 9, [(VBR, 50.0, 0.0), (7, 50.0, 0.0)]]
    for bad in ((np.nan, 0.0), (0.0, 0.0), (64.0, -0.5)):
        t = good_table.copy(); t[2] = bad
        refused.append([(VBR, 50.0, 0.0), t])
    refused += [[(CBR, np.nan, 0.0)], [(CBR, 0.0, 0.0)], [(ABR, 64.0, -0.5)]]
    for rungs in refused:
        with pytest.raises(ulc.UlcError, match=r"\(-1\)"):
            a.encode_ladder(x1, rungs)
    assert a.last_rungs() == 3
    for x in (x1, x2):
        ao, ab, aw, ac = a.encode_ladder(x, good)
        bo, bb, bw, bc = b.encode_ladder(x, good)
        assert np.array_equal(aw, bw) and np.array_equal(ac.view(np.uint32), bc.view(np.uint32))
        _same_blocks(ao, ab, bo, bb, "behind refused calls")
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
ENC = os.path.join(ROOT, "oracle", "_ref", "ulcencodetool_amd")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
needs_tools = pytest.mark.skipif(not (os.path.exists(ENC) and os.path.exists(TOOL)),
                                 reason="ulcx-tool or the oracle/_ref tools not built (needs the reference tree at build time)")


def _inputs(tmp_path, names, specs, rate, ch):
    ins = []
    for i, (name, (sec, kind)) in enumerate(zip(names, specs)):
        n = int(sec * rate)
        pcm = synth_pcm(90 + i, n, ch, rate, transient=(kind == "transient"), seed=19)
        pcm16 = np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype(np.int16)
        p = tmp_path / f"{name}.wav"
        write_wav16(p, pcm16, rate)
        ins.append((p, pcm16))
    return ins


@needs_tools
def test_cli_ladder_writes_the_reference_tools_file_for_every_rung(tmp_path):
    rate, ch = 44100, 2
    ins = _inputs(tmp_path, "abc", [(0.9, "transient"), (0.5, "tone"), (1.2, "transient")], rate, ch)
    (a, _), (b, _), (c, _) = ins
    args = ["-50/64/96,0.41", str(a), "-rate:-80/48/96,0.2", str(b), str(c)]
    want = {"a": ["-50", "64", "96,0.41"], "b": ["-80", "48", "96,0.2"], "c": ["-80", "48", "96,0.2"]}
    got, many, ref = tmp_path / "got", tmp_path / "many", tmp_path / "ref"
    for d in (got, many, ref):
        d.mkdir()
    run_tool([TOOL, "encode", str(got)] + args)
    run_tool([TOOL, "encode", str(many), args[0], "-devices:2"] + args[1:])
    assert sorted(os.listdir(got)) == sorted(f"{n}.r{i}.ulc" for n in "abc" for i in range(3))
    for p, _ in ins:
        for i, arg in enumerate(want[p.stem]):
            name = f"{p.stem}.r{i}.ulc"
            run_tool([ENC, str(p), str(ref / name), arg])
            r = open(ref / name, "rb").read()
            assert open(got / name, "rb").read() == r, f"{name} at {arg}: differs from ulcencodetool"
            assert open(many / name, "rb").read() == r, f"{name} at {arg}: -devices:2 changed the file"


@needs_tools
def test_cli_ladder_with_an_auto_rung_uses_each_files_own_average_complexity(tmp_path):
    rate, ch, bs = 44100, 2, 2048
    ins = _inputs(tmp_path, "xy", [(1.1, "transient"), (0.6, "tone")], rate, ch)
    got, ref = tmp_path / "got", tmp_path / "ref"
    got.mkdir(); ref.mkdir()
    out = run_tool([TOOL, "encode", str(got), "64,auto/-50"] + [str(p) for p, _ in ins]).stdout.decode()
    printed = {m.group(1): m.group(2) for m in re.finditer(r"^(\S+?): .*ABR complexity (\S+?)(?: \(CBR\))?(?:[,;]|$)", out, re.M)}
    for p, pcm16 in ins:
        n = pcm16.shape[0]
        nblk = (n + bs - 1) // bs + 2                                   # ulcEncodeTool.c:93-98
        x = np.zeros((nblk * bs, ch), np.float32)
        x[:n] = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
        first = oracle_encode_debug(x, bs, rate, 0, 50.0)
        avg = np.float32(sum(float(c) for c in first["cplx"]) / nblk)     # double sum in block order, then (float)
        assert np.float32(float(printed[p.name])) == avg, f"{p.name}: printed complexity {printed[p.name]} != {avg!r}"
        for i, arg in enumerate([f"64,{float(avg):.9g}", "-50"]):
            name = f"{p.stem}.r{i}.ulc"
            run_tool([ENC, str(p), str(ref / name), arg])
            assert open(got / name, "rb").read() == open(ref / name, "rb").read(), f"{name}: reference tool at {arg}"
