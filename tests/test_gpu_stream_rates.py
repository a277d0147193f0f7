"""Per-stream rate settings in one batched call (include/ulc_amd.h ulcx_encode_*_rates, ulcx-tool -rate: / RATE,auto).
Every stream of a mixed batch must be encoded exactly as the oracle's ULC_EncodeBlock_{VBR,CBR,ABR} restatement encodes it
with that stream's setting (one orc_encoder per stream, tests/rates_testlib.py), and exactly as the scalar API encodes it
in a uniform batch; the command line must write what the reference's tool writes file by file."""
import os
import re
import struct
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from ulc_testlib import write_wav16, run_tool
from gpu_testlib import amd as _ulc
from ulc_testlib import synth_pcm, oracle_encode_debug
from rates_testlib import oracle_streams, mode_of

pytestmark = pytest.mark.gpu

# (RateKbps, AvgComplexity) in the tool's convention: VBR at quality 1 / 37.5 / 50 / 100 / 117, CBR at 32 / 64 / 229 kbps,
# ABR at (64, 0.02), (64, 0.35), (128, 0.98)
MIXED = [(-1.0, 0.0), (32.0, 0.0), (64.0, 0.02), (-37.5, 0.0), (64.0, 0.0), (-50.0, 0.0), (64.0, 0.35), (-100.0, 0.0),
         (229.0, 0.0), (-117.0, 0.0), (128.0, 0.98), (-50.0, 0.3)]


def _batch_pcm(B, n, ch, rate, seed):
    return np.stack([synth_pcm(s, n, ch, rate, transient=(s % 3 != 1), seed=seed) for s in range(B)])


def _encode_calls(enc, pcm, bs, schedule, fetch=True):
    """One encode_rates call per entry of schedule (settings [B]); K blocks each.  Returns per-call results (+ taps)."""
    calls = len(schedule)
    K = pcm.shape[1] // (calls * bs)
    res = []
    for j, table in enumerate(schedule):
        out, bits, wc, cplx = enc.encode_rates(pcm[:, j * K * bs:(j + 1) * K * bs], np.array(table, np.float32))
        taps = enc.debug_fetch(K, parts=("keep", "nout")) if fetch else None
        res.append((out, bits, wc, cplx, taps))
    return res, K


def _check_against_oracle(res, K, ref, what):
    for j, (out, bits, wc, cplx, taps) in enumerate(res):
        for s in range(out.shape[0]):
            for k in range(K):
                o = ref[s][j * K + k]
                tag = f"{what}: stream {s} call {j} block {k}"
                assert bits[s, k] == o["bits"], f"{tag}: bits {bits[s, k]} != oracle {o['bits']}"
                assert wc[s, k] == o["wc"], f"{tag}: WindowCtrl"
                assert cplx[s, k].view(np.uint32) == o["cplx"].view(np.uint32), f"{tag}: BlockComplexity"
                assert np.array_equal(out[s, k, :bits[s, k] // 8], o["bytes"]), f"{tag}: bytes differ"
                if taps is not None:
                    assert taps["nout"][s, k] == o["nout"], f"{tag}: nOutCoef {taps['nout'][s, k]} != {o['nout']}"
                    assert np.array_equal(taps["keep"][s, k], o["keep"]), f"{tag}: kept set differs"


@pytest.mark.parametrize("force", [0, 2])
def test_mixed_batch_is_bit_exact_per_stream(force):
    """Stereo BlockSize 2048 at 44.1 kHz, twelve streams of every kind, K = 4, two calls; force = 2 sends every second block
    through the exact (heapsort-rank) path, VBR blocks of the mixed batch included."""
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, len(MIXED)
    pcm = _batch_pcm(B, 2 * K * bs, ch, rate, seed=31)
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    if force:
        enc.force_exact(force)
    res, K2 = _encode_calls(enc, pcm, bs, [MIXED, MIXED])
    if force:
        assert enc.last_fallbacks() > 0
    ref = oracle_streams(pcm, bs, rate, [MIXED, MIXED])
    _check_against_oracle(res, K2, ref, f"mixed (force_exact {force})")
    enc.close()


def test_mixed_batch_equals_the_scalar_api_stream_by_stream():
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 3, len(MIXED)
    pcm = _batch_pcm(B, 2 * K * bs, ch, rate, seed=32)
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    mixed = [enc.encode_rates(pcm[:, j * K * bs:(j + 1) * K * bs], np.array(MIXED, np.float32)) for j in range(2)]
    for s, setting in enumerate(MIXED):
        mode, p0, p1 = mode_of(setting)
        uni = ulc.BatchEncoder(B, ch, bs, rate, K)
        for j in range(2):
            out, bits, wc, cplx = uni.encode(pcm[:, j * K * bs:(j + 1) * K * bs], mode, p0, p1)
            mo, mb, mw, mc = mixed[j]
            assert np.array_equal(mb[s], bits[s]) and np.array_equal(mw[s], wc[s]), f"stream {s} {setting}: sizes / windows"
            assert np.array_equal(mc[s].view(np.uint32), cplx[s].view(np.uint32)), f"stream {s}: complexity"
            for k in range(K):
                assert np.array_equal(mo[s, k, :mb[s, k] // 8], out[s, k, :bits[s, k] // 8]), f"stream {s} {setting} call {j} block {k}"
        uni.close()
    enc.close()


def test_setting_changes_between_calls_with_the_table_rewritten_on_the_device():
    """VBR -> CBR -> ABR -> VBR per stream (rotated over the streams), the device table rewritten between calls by an
    asynchronous copy on the encoder's stream; every block against the per-block oracle."""
    import torch
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 48000, 2, 8
    cycle = [(-50.0, 0.0), (64.0, 0.0), (96.0, 0.3), (-80.0, 0.0)]
    schedule = [[cycle[(j + s) % 4] for s in range(B)] for j in range(4)]
    pcm = _batch_pcm(B, 4 * K * bs, ch, rate, seed=33)
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    d_rate = torch.zeros((B, 2), dtype=torch.float32, device=dev)
    d_out = torch.zeros((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((B, K), dtype=torch.int32, device=dev)
    d_wc = torch.zeros((B, K), dtype=torch.int32, device=dev)
    d_cplx = torch.zeros((B, K), dtype=torch.float32, device=dev)
    res = []
    for j in range(4):
        d_pcm = torch.from_numpy(np.ascontiguousarray(pcm[:, j * K * bs:(j + 1) * K * bs])).to(dev)
        h = torch.tensor(schedule[j], dtype=torch.float32).pin_memory()
        d_rate.copy_(h, non_blocking=True)
        enc.encode_dev_rates(d_rate.data_ptr(), d_pcm.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), d_wc.data_ptr(),
                             d_cplx.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        taps = enc.debug_fetch(K, parts=("keep", "nout"))
        res.append((d_out.cpu().numpy(), d_bits.cpu().numpy(), d_wc.cpu().numpy(), d_cplx.cpu().numpy(), taps))
    ref = oracle_streams(pcm, bs, rate, schedule)
    _check_against_oracle(res, K, ref, "changing settings")
    enc.close()


@pytest.mark.parametrize("ch,bs,rate,transient", [(1, 256, 44100, True), (2, 4096, 48000, True), (6, 1024, 44100, False)])
def test_other_geometries(ch, bs, rate, transient):
    """Mono 256, stereo 4096 at 48 kHz with window switching (the benched wswitch shape: k_select_pair), six channels."""
    ulc = _ulc()
    K, B = 3, 7
    table = [(-50.0, 0.0), (48.0, 0.0), (-90.0, 0.0), (128.0, 0.5), (32.0, 0.0), (-20.0, 0.0), (64.0, 0.2)]
    pcm = np.stack([synth_pcm(s, 2 * K * bs, ch, rate, transient=transient, seed=34) for s in range(B)])
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    res, K2 = _encode_calls(enc, pcm, bs, [table, table])
    ref = oracle_streams(pcm, bs, rate, [table, table])
    _check_against_oracle(res, K2, ref, f"{ch}ch BlockSize {bs}")
    enc.close()


def test_pcm16_ingest_equals_float_ingest():
    import torch
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, len(MIXED)
    pcm = _batch_pcm(B, K * bs, ch, rate, seed=35)
    pcm16 = np.clip(np.rint(pcm * 32768.0), -32768, 32767).astype(np.int16)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    d_rate = torch.tensor(MIXED, dtype=torch.float32, device=dev)
    outs = []
    for use16 in (False, True):
        enc = ulc.BatchEncoder(B, ch, bs, rate, K)
        d_in = torch.from_numpy(pcm16).to(dev) if use16 else torch.from_numpy(pcm16.astype(np.float32) * np.float32(2.0 ** -15)).to(dev)
        d_out = torch.zeros((B, K, enc.slot), dtype=torch.uint8, device=dev)
        d_bits = torch.zeros((B, K), dtype=torch.int32, device=dev)
        d_cplx = torch.zeros((B, K), dtype=torch.float32, device=dev)
        enc.encode_dev_rates(d_rate.data_ptr(), d_in.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), 0, d_cplx.data_ptr(),
                             stream=st.cuda_stream, pcm16=use16)
        st.synchronize()
        bits = d_bits.cpu().numpy()
        out = d_out.cpu().numpy()
        outs.append((bits, [out[s, k, :bits[s, k] // 8].tobytes() for s in range(B) for k in range(K)], d_cplx.cpu().numpy()))
        enc.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32))


@pytest.mark.parametrize("table,mode,p0,rate", [((-50.0, 0.0), 0, 50.0, 44100), ((64.0, 0.0), 1, 64.0, 48000)])
def test_uniform_tables_equal_the_scalar_call(table, mode, p0, rate):
    ulc = _ulc()
    bs, ch, K, B = 2048, 2, 4, 16
    pcm = _batch_pcm(B, 2 * K * bs, ch, rate, seed=36)
    a = ulc.BatchEncoder(B, ch, bs, rate, K)
    b = ulc.BatchEncoder(B, ch, bs, rate, K)
    for j in range(2):
        x = pcm[:, j * K * bs:(j + 1) * K * bs]
        ro, rb, rw, rc = a.encode_rates(x, np.array([table] * B, np.float32))
        so, sb, sw, sc = b.encode(x, mode, p0, 0.0)
        assert np.array_equal(rb, sb) and np.array_equal(rw, sw) and np.array_equal(rc.view(np.uint32), sc.view(np.uint32))
        for s in range(B):
            for k in range(K):
                assert np.array_equal(ro[s, k, :rb[s, k] // 8], so[s, k, :sb[s, k] // 8]), f"stream {s} call {j} block {k}"
    a.close(); b.close()


def test_host_validation_refuses_bad_entries_before_any_device_work():
    """A NaN, a zero rate or a negative complexity: ULCX_ERR_ARG, and the encoder's state is untouched (the next valid call
    gives the bytes it gives without the refused call in between)."""
    ulc = _ulc()
    bs, ch, rate, K, B = 1024, 2, 44100, 2, 4
    good = np.array([(-50.0, 0.0), (64.0, 0.0), (96.0, 0.3), (-70.0, 0.0)], np.float32)
    pcm = _batch_pcm(B, 3 * K * bs, ch, rate, seed=37)
    a = ulc.BatchEncoder(B, ch, bs, rate, K)
    b = ulc.BatchEncoder(B, ch, bs, rate, K)
    x0, x1, x2 = (pcm[:, j * K * bs:(j + 1) * K * bs] for j in range(3))
    a.encode_rates(x0, good); b.encode_rates(x0, good)
    for bad in ((np.nan, 0.0), (64.0, np.nan), (np.inf, 0.0), (0.0, 0.0), (-0.0, 0.0), (64.0, -0.5)):
        t = good.copy(); t[2] = bad
        with pytest.raises(ulc.UlcError, match=r"\(-1\)"):
            a.encode_rates(x1, t)
    for x in (x1, x2):
        ao, ab, aw, ac = a.encode_rates(x, good)
        bo, bb, bw, bc = b.encode_rates(x, good)
        assert np.array_equal(ab, bb) and np.array_equal(aw, bw) and np.array_equal(ac.view(np.uint32), bc.view(np.uint32))
        for s in range(B):
            for k in range(K):
                assert np.array_equal(ao[s, k, :ab[s, k] // 8], bo[s, k, :bb[s, k] // 8]), f"stream {s} block {k}"
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
ENC = os.path.join(ROOT, "oracle", "_ref", "ulcencodetool_amd")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
needs_tools = pytest.mark.skipif(not (os.path.exists(ENC) and os.path.exists(TOOL)),
                                 reason="ulcx-tool or the oracle/_ref tools not built (needs /root/reference at build time)")


def _inputs(tmp_path, specs, rate, ch):
    ins = []
    for i, (sec, kind) in enumerate(specs):
        n = int(sec * rate)
        if kind == "silent":
            pcm16 = np.zeros((n, ch), np.int16)
        else:
            pcm = synth_pcm(80 + i, n, ch, rate, transient=(kind == "transient"), seed=17)
            pcm16 = np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype(np.int16)
        p = tmp_path / f"f{i}.wav"
        write_wav16(p, pcm16, rate)
        ins.append((p, pcm16))
    return ins


@needs_tools
def test_cli_rate_groups_match_the_reference_tool_file_by_file(tmp_path):
    rate, ch = 44100, 2
    ins = _inputs(tmp_path, [(0.9, "transient"), (0.5, "tone"), (1.2, "transient"), (0.7, "tone"), (0.4, "transient")], rate, ch)
    args = ["-50", str(ins[0][0]), "-rate:48", str(ins[1][0]), str(ins[2][0]), "-rate:96,0.41", str(ins[3][0]), "-rate:-80", str(ins[4][0])]
    want = ["-50", "48", "48", "96,0.41", "-80"]
    got, ref = tmp_path / "got", tmp_path / "ref"
    got.mkdir(); ref.mkdir()
    run_tool([TOOL, "encode", str(got)] + args)
    many = tmp_path / "many"; many.mkdir()
    run_tool([TOOL, "encode", str(many), args[0], "-devices:2"] + args[1:])
    for (p, _), arg in zip(ins, want):
        run_tool([ENC, str(p), str(ref / (p.stem + ".ulc")), arg])
        r = open(ref / (p.stem + ".ulc"), "rb").read()
        assert open(got / (p.stem + ".ulc"), "rb").read() == r, f"{p.name} at {arg}: differs from ulcencodetool"
        assert open(many / (p.stem + ".ulc"), "rb").read() == r, f"{p.name} at {arg}: -devices:2 changed the file"


@needs_tools
def test_cli_two_pass_abr_uses_each_files_own_average_complexity(tmp_path):
    """`64,auto` over files of different length and character and a digitally silent one (complexity 0: CBR)."""
    rate, ch, bs = 44100, 2, 2048
    ins = _inputs(tmp_path, [(1.1, "transient"), (0.6, "tone"), (1.7, "transient"), (0.5, "silent")], rate, ch)
    got = tmp_path / "got"; got.mkdir()
    out = run_tool([TOOL, "encode", str(got), "64,auto"] + [str(p) for p, _ in ins]).stdout.decode()
    printed = {m.group(1): m.group(2) for m in re.finditer(r"^(\S+?): .*ABR complexity (\S+?)(?: \(CBR\))?, avg complexity", out, re.M)}
    for p, pcm16 in ins:
        n = pcm16.shape[0]
        nblk = (n + bs - 1) // bs + 2                                   # ulcEncodeTool.c:93-98
        x = np.zeros((nblk * bs, ch), np.float32)
        x[:n] = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
        first = oracle_encode_debug(x, bs, rate, 0, 50.0)
        avg = np.float32(sum(float(c) for c in first["cplx"]) / nblk)     # double sum in block order, then (float)
        assert np.float32(float(printed[p.name])) == avg, f"{p.name}: printed complexity {printed[p.name]} != {avg!r}"
        if p.stem == "f3":
            assert avg == 0.0
        ref = oracle_encode_debug(x, bs, rate, 2 if avg > 0 else 1, 64.0, float(avg), slot=2 * ch * bs + 16)
        sizes = (ref["bits"] + 7) // 8
        payload = b"".join(ref["out"][k, :sizes[k]].tobytes() for k in range(nblk))
        kbps = int(np.rint(int(sizes.sum()) * 8.0 * rate / 1000.0 / (bs * nblk)))
        want = struct.pack("<IHHIIHHI", 0x32434C55, bs, int(sizes.max()), nblk, rate, ch, kbps, 24) + payload
        assert open(got / (p.stem + ".ulc"), "rb").read() == want, f"{p.name}: two-pass ABR file differs from the oracle's"
        # and the reference tool, fed the same complexity, writes the same file
        refdir = tmp_path / "ref"; refdir.mkdir(exist_ok=True)
        run_tool([ENC, str(p), str(refdir / (p.stem + ".ulc")), f"64,{float(avg):.9g}"])
        assert open(refdir / (p.stem + ".ulc"), "rb").read() == want, f"{p.name}: reference tool at 64,{float(avg):.9g}"
