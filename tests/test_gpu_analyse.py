"""The analysis-only call (ulcx_analyse_dev / _dev_pcm16 / _host) on the GPU: window codes and block complexities bit for
bit against the oracle, the streams' state behind an analysis call (the next ENCODE call's bytes against the oracle's for
the uninterrupted stream), what the call leaves of a "last call", and the tool's `analyse` sub-command."""
import os
import re
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from ulc_testlib import write_wav16
from gpu_testlib import amd as _ulc
from ulc_testlib import synth_pcm, oracle_encode_debug
from rates_testlib import OracleStream

pytestmark = pytest.mark.gpu

# (BlockSize, channels, Hz, K)
GEOMETRIES = [(2048, 2, 44100, 12), (2048, 1, 44100, 12), (4096, 2, 48000, 10), (256, 2, 44100, 24), (1024, 3, 44100, 10),
              (512, 6, 48000, 10), (16384, 2, 44100, 4)]


def _batch_pcm(bs, ch, rate, K, seed=41, B=6):
    pcm = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=seed) for s in range(B)])
    pcm[B - 1] = 0.0                                              # digital silence: complexity exactly 0
    return pcm


def _oracle_series(pcm, bs, rate):
    """(wc[B][K], cplx[B][K]) of the oracle, one OracleStream per stream driven block by block (VBR 50: neither value
    depends on the rate mode)."""
    B, n, ch = pcm.shape
    K = n // bs
    wc = np.zeros((B, K), np.int32)
    cplx = np.zeros((B, K), np.float32)
    for s in range(B):
        o = OracleStream(ch, bs, rate)
        for k in range(K):
            r = o.block(pcm[s, k * bs:(k + 1) * bs], (-50.0, 0.0))
            wc[s, k], cplx[s, k] = r["wc"], r["cplx"]
        o.close()
    return wc, cplx


def _assert_not_trivial(wc, cplx):
    assert int((wc != 0x10).sum()) >= 4, "the oracle window-switches fewer than 4 blocks of this input"
    assert len(np.unique(cplx.view(np.uint32))) >= 10, "fewer than 10 distinct complexity values"
    assert int((cplx == 0.0).sum()) >= 1, "no block of complexity exactly 0"


def _assert_series(got_wc, got_cplx, wc, cplx, what):
    print(f"{what}: {int((wc != 0x10).sum())} window-switched, {len(np.unique(cplx.view(np.uint32)))} distinct complexities, "
          f"{int((got_wc != wc).sum())} wc mismatches, {int((got_cplx.view(np.uint32) != cplx.view(np.uint32)).sum())} complexity mismatches")
    assert np.array_equal(got_wc, wc), f"{what}: WindowCtrl differs from the oracle at {np.argwhere(got_wc != wc)[:4].tolist()}"
    bad = np.argwhere(got_cplx.view(np.uint32) != cplx.view(np.uint32))
    assert bad.size == 0, f"{what}: BlockComplexity differs from the oracle at {bad[:4].tolist()}"


@pytest.mark.parametrize("bs,ch,rate,K", GEOMETRIES)
def test_outputs_are_bit_exact_against_the_oracle(bs, ch, rate, K):
    ulc = _ulc()
    pcm = _batch_pcm(bs, ch, rate, K)
    wc, cplx = _oracle_series(pcm, bs, rate)
    _assert_not_trivial(wc, cplx)
    enc = ulc.BatchEncoder(pcm.shape[0], ch, bs, rate, K // 2)
    h = K // 2
    parts = [enc.analyse(pcm[:, j * h * bs:(j + 1) * h * bs]) for j in range(2)]
    enc.close()
    _assert_series(np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1), wc, cplx, f"BlockSize {bs} x {ch}")


def test_pcm16_ingest_against_the_oracle():
    import torch
    ulc = _ulc()
    bs, ch, rate, K = 2048, 2, 44100, 12
    pcm16 = np.clip(np.rint(_batch_pcm(bs, ch, rate, K) * 32768.0), -32768, 32767).astype(np.int16)
    x = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
    wc, cplx = _oracle_series(x, bs, rate)
    _assert_not_trivial(wc, cplx)
    B, h = pcm16.shape[0], K // 2
    dev = torch.device("cuda:0")
    enc = ulc.BatchEncoder(B, ch, bs, rate, h)
    d_wc = torch.zeros((B, h), dtype=torch.int32, device=dev)
    d_cplx = torch.zeros((B, h), dtype=torch.float32, device=dev)
    got = []
    for j in range(2):
        d_pcm = torch.from_numpy(np.ascontiguousarray(pcm16[:, j * h * bs:(j + 1) * h * bs])).to(dev)
        enc.analyse_dev(d_pcm.data_ptr(), h, d_wc.data_ptr(), d_cplx.data_ptr(), pcm16=True)
        torch.cuda.synchronize()
        got.append((d_wc.cpu().numpy(), d_cplx.cpu().numpy()))
    enc.close()
    _assert_series(np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1), wc, cplx, "PCM16 ingest")


def test_equals_the_encode_call():
    ulc = _ulc()
    bs, ch, rate, K = 2048, 2, 44100, 12
    pcm = _batch_pcm(bs, ch, rate, K)
    wc, cplx = _oracle_series(pcm, bs, rate)
    B, h = pcm.shape[0], K // 2
    e1, e2 = ulc.BatchEncoder(B, ch, bs, rate, h), ulc.BatchEncoder(B, ch, bs, rate, h)
    for j in range(2):
        x = pcm[:, j * h * bs:(j + 1) * h * bs]
        _, _, ewc, ecplx = e1.encode(x, ulc.MODE_VBR, 50.0)
        awc, acplx = e2.analyse(x)
        assert np.array_equal(ewc, awc), f"call {j}: WindowCtrl of encode and analyse differ"
        assert np.array_equal(ecplx.view(np.uint32), acplx.view(np.uint32)), f"call {j}: BlockComplexity of encode and analyse differ"
        _assert_series(awc, acplx, wc[:, j * h:(j + 1) * h], cplx[:, j * h:(j + 1) * h], f"call {j}")
    e1.close(); e2.close()


def _assert_blocks(out, bits, wc, ref, k0, K, what):
    """out/bits/wc [K] of one stream against blocks k0 .. k0+K-1 of the oracle's stream"""
    for k in range(K):
        tag = f"{what}: block {k0 + k}"
        assert bits[k] == ref["bits"][k0 + k], f"{tag}: size {bits[k]} != oracle {ref['bits'][k0 + k]}"
        assert wc[k] == ref["wc"][k0 + k], f"{tag}: WindowCtrl"
        nb = bits[k] // 8
        assert np.array_equal(out[k, :nb], ref["out"][k0 + k, :nb]), f"{tag}: bytes differ from the oracle's"


@pytest.mark.parametrize("bs,rate", [(2048, 44100), (4096, 48000)])
@pytest.mark.parametrize("mode,p0", [(1, 64.0), (0, 50.0)])
def test_state_behind_an_analysis_call(bs, rate, mode, p0):
    ulc = _ulc()
    ch, K, B = 2, 5, 4
    pcm = np.stack([synth_pcm(s, 3 * K * bs, ch, rate, transient=True, seed=42) for s in range(B)])
    ref = [oracle_encode_debug(pcm[s], bs, rate, mode, p0) for s in range(B)]
    assert sum(int((r["wc"] != 0x10).sum()) for r in ref) >= 4
    seg = [pcm[:, j * K * bs:(j + 1) * K * bs] for j in range(3)]
    # analyse blocks 0..K-1, then ENCODE blocks K..2K-1
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    awc, acplx = enc.analyse(seg[0])
    out, bits, wc, cplx = enc.encode(seg[1], mode, p0)
    for s in range(B):
        assert np.array_equal(awc[s], ref[s]["wc"][:K]) and np.array_equal(acplx[s].view(np.uint32), ref[s]["cplx"][:K].view(np.uint32))
        _assert_blocks(out[s], bits[s], wc[s], ref[s], K, K, f"analyse/encode stream {s}")
        assert np.array_equal(cplx[s].view(np.uint32), ref[s]["cplx"][K:2 * K].view(np.uint32))
    # analyse, reset, encode = a fresh encoder
    enc.reset()
    out, bits, wc, cplx = enc.encode(seg[0], mode, p0)
    for s in range(B):
        _assert_blocks(out[s], bits[s], wc[s], ref[s], 0, K, f"analyse/reset/encode stream {s}")
    # encode / analyse / encode (continuing behind the encode call above)
    awc, acplx = enc.analyse(seg[1])
    out, bits, wc, cplx = enc.encode(seg[2], mode, p0)
    for s in range(B):
        assert np.array_equal(awc[s], ref[s]["wc"][K:2 * K]) and np.array_equal(acplx[s].view(np.uint32), ref[s]["cplx"][K:2 * K].view(np.uint32))
        _assert_blocks(out[s], bits[s], wc[s], ref[s], 2 * K, K, f"encode/analyse/encode stream {s}")
    enc.close()


def test_no_last_call_is_left_behind():
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 4, 3
    pcm = np.stack([synth_pcm(s, 2 * K * bs, ch, rate, transient=True, seed=43) for s in range(B)])
    ref = [oracle_encode_debug(pcm[s], bs, rate, 0, 50.0) for s in range(B)]
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    enc.force_exact(2)
    enc.encode(pcm[:, :K * bs], ulc.MODE_VBR, 50.0)
    assert enc.last_fallbacks() > 0
    enc.reset()
    enc.analyse(pcm[:, :K * bs])
    with pytest.raises(ulc.UlcError):
        enc.debug_fetch(K, parts=("coef",))
    assert enc.last_fallbacks() == 0
    ms = enc.stage_ms()
    assert set(ms) == {ulc.lib().ulcx_encoder_stage_name(i).decode() for i in range(21)}
    assert ms["k_xf"] > 0.0 and ms["k_cplx"] > 0.0
    for name in ("k_pbark", "k_select", "k_nsums", "k_tails", "k_encode_wave", "k_encode_units", "k_pack", "cbr_probe_passes"):
        assert ms[name] == 0.0, name
    enc.force_exact(0)
    out, bits, wc, cplx = enc.encode(pcm[:, K * bs:], ulc.MODE_VBR, 50.0)
    taps = enc.debug_fetch(K, parts=("coef", "keep", "nout"))
    assert enc.last_fallbacks() >= 0
    for s in range(B):
        _assert_blocks(out[s], bits[s], wc[s], ref[s], K, K, f"stream {s}")
        assert np.array_equal(taps["coef"][s], ref[s]["coef"][K:]), f"stream {s}: coefficients"
        assert np.array_equal(taps["nout"][s], ref[s]["nout"][K:]), f"stream {s}: nOutCoef"
        assert np.array_equal(taps["keep"][s], (ref[s]["ranks"][K:] < ref[s]["nout"][K:, None]).astype(np.uint8)), f"stream {s}: kept set"
    enc.close()


def test_benched_shape_once():
    import torch
    ulc = _ulc()
    bs, ch, rate, K, B = 2048, 2, 44100, 32, 4096
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    d_wc = torch.zeros((B, K), dtype=torch.int32, device=dev)
    d_cplx = torch.zeros((B, K), dtype=torch.float32, device=dev)
    enc = ulc.BatchEncoder(B, ch, bs, rate, K)
    enc.analyse_dev(d_pcm.data_ptr(), K, d_wc.data_ptr(), d_cplx.data_ptr())
    torch.cuda.synchronize()
    enc.close()
    gwc, gcplx = d_wc.cpu().numpy(), d_cplx.cpu().numpy()
    streams = [0, 1, 5, 15, 16, 2049, 4090, 4095]
    wc, cplx = _oracle_series(base[[s % 16 for s in streams]], bs, rate)
    _assert_series(gwc[streams], gcplx[streams], wc, cplx, "4096 x 32 x 2048")
    # the batch is 16 streams tiled: every copy must agree with its original
    assert np.array_equal(gwc, gwc[np.arange(B) % 16]) and np.array_equal(gcplx.view(np.uint32), gcplx.view(np.uint32)[np.arange(B) % 16])


def test_device_pointers_on_a_side_stream_one_output_at_a_time():
    import torch
    ulc = _ulc()
    bs, ch, rate, K = 2048, 2, 48000, 12
    pcm = _batch_pcm(bs, ch, rate, K)
    wc, cplx = _oracle_series(pcm, bs, rate)
    _assert_not_trivial(wc, cplx)
    B, h = pcm.shape[0], K // 2
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    enc = ulc.BatchEncoder(B, ch, bs, rate, h)
    with torch.cuda.stream(st):
        d_wc = torch.full((B, h), -1, dtype=torch.int32, device=dev)
        d_cplx = torch.full((B, h), -1.0, dtype=torch.float32, device=dev)
        d0 = torch.from_numpy(np.ascontiguousarray(pcm[:, :h * bs])).to(dev)
        d1 = torch.from_numpy(np.ascontiguousarray(pcm[:, h * bs:])).to(dev)
        enc.analyse_dev(d0.data_ptr(), h, 0, d_cplx.data_ptr(), stream=st.cuda_stream)        # complexities only
        enc.analyse_dev(d1.data_ptr(), h, d_wc.data_ptr(), 0, stream=st.cuda_stream)          # window codes only
        st.synchronize()
    gwc, gcplx = d_wc.cpu().numpy(), d_cplx.cpu().numpy()
    enc.close()
    assert np.array_equal(gcplx.view(np.uint32), cplx[:, :h].view(np.uint32)), "complexities of the first call"
    assert np.array_equal(gwc, wc[:, h:]), "window codes of the second call (the state behind a complexities-only call)"


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")


@pytest.mark.parametrize("devices", [1, 2])
def test_cli_analyse_prints_the_average_complexity_of_each_file(tmp_path, devices):
    rate, ch, bs = 44100, 2, 2048
    work = tmp_path / "in"; work.mkdir()
    ins = []
    for i, (sec, kind) in enumerate([(1.1, "transient"), (0.6, "tone"), (0.5, "silent")]):
        n = int(sec * rate)
        if kind == "silent":
            pcm16 = np.zeros((n, ch), np.int16)
        else:
            pcm16 = np.clip(np.rint(synth_pcm(80 + i, n, ch, rate, transient=(kind == "transient"), seed=17) * 32767.0), -32768, 32767).astype(np.int16)
        write_wav16(work / f"f{i}.wav", pcm16, rate)
        ins.append((work / f"f{i}.wav", pcm16))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "ulc-codec_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    cwd = tmp_path / "cwd"; cwd.mkdir()
    p = subprocess.run([TOOL, "analyse", f"-devices:{devices}"] + [str(f) for f, _ in ins], capture_output=True, env=env, cwd=str(cwd), timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-400:]
    got = {m.group(1): (int(m.group(2)), m.group(3), int(m.group(4)))
           for m in re.finditer(r"^(\S+?): (\d+) blocks, avg complexity (\S+), (\d+) window-switched$", p.stdout.decode(), re.M)}
    assert os.listdir(str(cwd)) == [] and sorted(os.listdir(str(work))) == ["f0.wav", "f1.wav", "f2.wav"], "the sub-command wrote a file"
    for f, pcm16 in ins:
        n = pcm16.shape[0]
        nblk = (n + bs - 1) // bs + 2                                   # ulcEncodeTool.c:93-98
        x = np.zeros((1, nblk * bs, ch), np.float32)
        x[0, :n] = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
        wc, cplx = _oracle_series(x, bs, rate)
        avg = np.float32(sum(float(c) for c in cplx[0]) / nblk)         # double sum in block order, then (float): what RATE,auto uses
        assert got[f.name] == (nblk, "%.9g" % float(avg), int((wc[0] != 0x10).sum())), f"{f.name}: {got[f.name]}"
    assert got["f2.wav"][1] == "0"
