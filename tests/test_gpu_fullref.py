"""The HIP kernels against the REAL reference (all seven libulc sources over the project's standin/Fourier.h, built by
oracle/Makefile into oracle/_ref/ where the reference tree is present): batched encodes and decodes through the C ABI against
oracle/_ref/ulc_ref_driver, one stream per driver process, and the reference's own tools over libulc_amd.so against the same
tools over the full reference build, file for file.  Only oracle/_ref/ build outputs are read.  The transforms on the
reference side are the project's spec v2 (refereed in float64 elsewhere); everything else is the real code."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
from fullref_cases import ENC_CASES, DEC_ONLY, enc_case, have_driver, driver_encode, driver_decode, REF_DIR  # noqa: E402
from ulc_testlib import synth_pcm, run_tool  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_driver(), reason="oracle/_ref/ulc_ref_driver not built (reference tree absent at build time)")]
COMPARED = {"streams": 0, "blocks": 0, "decoder streams": 0, "decoder blocks": 0}


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    yield
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    line = "gpu fullref: compared with the real reference: %(streams)d encoder streams / %(blocks)d blocks, " \
           "%(decoder streams)d decoder streams / %(decoder blocks)d blocks" % COMPARED
    tr.write_line(line) if tr is not None else print(line)


def _groups():
    """Encoder cases that share a shape and rate-control setting, batched together (at most 8 streams per batch)."""
    g = {}
    for tag in sorted(ENC_CASES):
        pcm, bs, rate, mode, p0, p1 = enc_case(tag)
        g.setdefault((bs, pcm.shape[1], rate, mode, p0, p1, pcm.shape[0] // bs), []).append(tag)
    out = []
    for key, tags in sorted(g.items(), key=lambda kv: kv[1][0]):
        for i in range(0, len(tags), 8):
            out.append((key, tuple(tags[i:i + 8])))
    return out


GROUPS = _groups()


def _encode_dev(amd, torch, pcm, bs, rate, mode, p0, p1, calls):
    """pcm [B][K*bs][C] through ulcx_encode_dev in `calls` pieces, state carried -> numpy (out, bits, wc, cplx)."""
    B, n, ch = pcm.shape
    K = n // bs
    cuts = np.linspace(0, K, calls + 1).astype(int)
    enc = amd.BatchEncoder(B, ch, bs, rate, int(np.diff(cuts).max()))
    dev = torch.device("cuda", 0)
    outs = []
    for c in range(calls):
        k0, k1 = int(cuts[c]), int(cuts[c + 1])
        if k1 == k0:
            continue
        d_pcm = torch.from_numpy(np.ascontiguousarray(pcm[:, k0 * bs:k1 * bs])).to(dev)
        out = torch.zeros(B, k1 - k0, enc.slot, dtype=torch.uint8, device=dev)
        bits = torch.zeros(B, k1 - k0, dtype=torch.int32, device=dev)
        wc = torch.zeros_like(bits); cplx = torch.zeros(B, k1 - k0, dtype=torch.float32, device=dev)
        enc.encode_dev(d_pcm.data_ptr(), k1 - k0, out.data_ptr(), bits.data_ptr(), wc.data_ptr(), cplx.data_ptr(), mode=mode, p0=p0, p1=p1)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (out, bits, wc, cplx)])
    enc.close()
    return [np.concatenate([o[i] for o in outs], axis=1) for i in range(4)]


def _decode_dev(amd, torch, blocks, ch, bs):
    """blocks [B][K][slot] through ulcx_decode_dev in one call -> numpy (pcm [B][K*bs][C], bits [B][K])."""
    B, K, slot = blocks.shape
    dev = torch.device("cuda", 0)
    dec = amd.BatchDecoder(B, ch, bs, K)
    d_in = torch.from_numpy(np.ascontiguousarray(blocks)).to(dev)
    pcm = torch.zeros(B, K * bs, ch, dtype=torch.float32, device=dev); bits = torch.zeros(B, K, dtype=torch.int32, device=dev)
    dec.decode_dev(d_in.data_ptr(), slot, K, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    r = pcm.cpu().numpy(), bits.cpu().numpy()
    dec.close()
    return r


def _check_stream(what, ref, out, bits, wc, cplx):
    for k in range(len(ref["bits"])):
        assert wc[k] == ref["wc"][k], f"{what} block {k}: WindowCtrl {wc[k]:#x}, real {ref['wc'][k]:#x}"
        assert cplx[k].tobytes() == ref["cplx"][k].tobytes(), f"{what} block {k}: BlockComplexity {cplx[k]}, real {ref['cplx'][k]}"
        assert bits[k] == ref["bits"][k], f"{what} block {k}: size {bits[k]}, real {ref['bits'][k]}"
        nb = (int(bits[k]) + 7) // 8
        assert out[k, :nb].tobytes() == ref["out"][k, :nb].tobytes(), f"{what} block {k}: bytes differ from the real reference's"


@pytest.mark.parametrize("key,tags", GROUPS, ids=[t[0] for _, t in GROUPS])
def test_batched_encode_and_decode_equal_the_real_reference(key, tags):
    import torch
    import ulc_amd as amd
    bs, ch, rate, mode, p0, p1, K = key
    pcm = np.stack([enc_case(t)[0] for t in tags])
    refs = [driver_encode(pcm[i], bs, rate, mode, p0, p1) for i in range(len(tags))]
    out, bits, wc, cplx = _encode_dev(amd, torch, pcm, bs, rate, mode, p0, p1, calls=min(3, K))
    for i, t in enumerate(tags):
        _check_stream(t, refs[i], out[i], bits[i], wc[i], cplx[i])
        COMPARED["streams"] += 1; COMPARED["blocks"] += K
    # the real encoder's streams through the device decoder: every batched stream's noise generator starts fresh
    blocks = np.stack([r["out"] for r in refs])
    dpcm, dbits = _decode_dev(amd, torch, blocks, ch, bs)
    for i, t in enumerate(tags):
        rbits, rpcm = driver_decode(refs[i]["out"], ch, bs)
        assert np.array_equal(dbits[i], rbits), f"{t}: bits read differ from the real decoder's"
        assert dpcm[i].view(np.uint32).tobytes() == rpcm.view(np.uint32).tobytes(), f"{t}: decoded PCM differs from the real decoder's"
        COMPARED["decoder streams"] += 1; COMPARED["decoder blocks"] += K


@pytest.mark.parametrize("tag", sorted(DEC_ONLY))
def test_device_decoder_equals_the_real_decoder_on_assembled_streams(tag):
    """Every header code, every code the format allocates, and the opening-Fh unit; two copies in one batch (each starts its
    noise generator fresh, as a fresh reference process does)."""
    import torch
    import ulc_amd as amd
    blocks, bs, ch = DEC_ONLY[tag]()
    rbits, rpcm = driver_decode(blocks, ch, bs)
    dpcm, dbits = _decode_dev(amd, torch, np.stack([blocks, blocks]), ch, bs)
    for s in range(2):
        assert np.array_equal(dbits[s], rbits)
        assert dpcm[s].view(np.uint32).tobytes() == rpcm.view(np.uint32).tobytes(), f"copy {s}: PCM differs from the real decoder's"
        COMPARED["decoder streams"] += 1; COMPARED["decoder blocks"] += len(rbits)


@pytest.mark.parametrize("name", ["vbr50", "cbr64_48k", "wswitch_4096"])
def test_benched_inputs_sampled_against_the_real_reference(name):
    """Each bench.CONFIGS input at its benched shape (one GPU: per_gpu or total streams), encoded and decoded in one call each
    as bench.py does; 8 seeded streams - two from the decoder's cut last round - against the driver."""
    import torch
    import ulc_amd as amd
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS[name]
    B, K, bs, ch, rate = cfg["per_gpu"] or cfg["total"], cfg["blocks"], cfg["bs"], bench.CH, cfg["rate"]
    mode = amd.MODE_VBR if cfg["mode"] == "vbr" else amd.MODE_CBR
    dev = torch.device("cuda", 0)
    keep = bench.RATE
    bench.RATE = rate
    try:
        pcm = bench.make_pcm(torch, B, K * bs, dev, seed=1234, bursts_per_s=cfg["bursts"], decades=cfg["decades"])
    finally:
        bench.RATE = keep
    enc = amd.BatchEncoder(B, ch, bs, rate, K); dec = amd.BatchDecoder(B, ch, bs, K)
    slot = enc.slot
    out = torch.zeros(B, K, slot, dtype=torch.uint8, device=dev); bits = torch.zeros(B, K, dtype=torch.int32, device=dev)
    wc = torch.zeros_like(bits); cplx = torch.zeros(B, K, dtype=torch.float32, device=dev)
    dpcm = torch.zeros(B, K * bs, ch, dtype=torch.float32, device=dev); dbits = torch.zeros_like(bits)
    enc.encode_dev(pcm.data_ptr(), K, out.data_ptr(), bits.data_ptr(), wc.data_ptr(), cplx.data_ptr(), mode=mode, p0=cfg["p0"])
    dec.decode_dev(out.data_ptr(), slot, K, dpcm.data_ptr(), dbits.data_ptr())
    torch.cuda.synchronize()
    grid, whole, resident = dec.last_cut()
    enc.close(); dec.close()
    first_cut = whole if grid else (B - B % resident if resident else 3 * B // 4)
    first_cut = min(first_cut, B - 2)
    rng = np.random.default_rng(7)
    sample = sorted(set(rng.choice(first_cut, 6, replace=False).tolist()) | set((first_cut + rng.choice(B - first_cut, 2, replace=False)).tolist()))
    assert len(sample) == 8 and sum(s >= first_cut for s in sample) >= 2
    idx = torch.tensor(sample, device=dev)
    pcm_h = pcm[idx].cpu().numpy(); out_h = out[idx].cpu().numpy(); bits_h = bits[idx].cpu().numpy()
    wc_h = wc[idx].cpu().numpy(); cplx_h = cplx[idx].cpu().numpy(); dp_h = dpcm[idx].cpu().numpy(); db_h = dbits[idx].cpu().numpy()
    del pcm, out, dpcm
    for i, s in enumerate(sample):
        ref = driver_encode(pcm_h[i], bs, rate, mode, cfg["p0"], 0.0, slot=slot)
        _check_stream(f"{name} stream {s}", ref, out_h[i], bits_h[i], wc_h[i], cplx_h[i])
        rbits, rpcm = driver_decode(ref["out"], ch, bs)
        assert np.array_equal(db_h[i], rbits), s
        assert dp_h[i].view(np.uint32).tobytes() == rpcm.view(np.uint32).tobytes(), f"{name} stream {s}: decoded PCM differs from the real decoder's"
        COMPARED["streams"] += 1; COMPARED["blocks"] += K; COMPARED["decoder streams"] += 1; COMPARED["decoder blocks"] += K


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_DIR, "ulcencodetool_amd")), reason="_amd tools not built")
@pytest.mark.parametrize("ch,rate,seconds,arg", [
    (2, 44100, 1.5, "-50"),          # VBR
    (2, 48000, 1.5, "64"),           # CBR
    (2, 44100, 1.5, "64,0.35"),      # ABR
    (6, 48000, 0.8, "-60"),          # 5.1
])
def test_reference_tools_over_libulc_amd_write_the_real_references_files(ch, rate, seconds, arg, tmp_path):
    import wave
    pcm = synth_pcm(5, int(seconds * rate), ch, rate, transient=True, seed=19)
    wav = tmp_path / "in.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(ch); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.clip(np.rint(pcm * 32767.0), -32768, 32767).astype("<i2").tobytes())
    files = {}
    for side in ("amd", "ref"):
        ulc, f32, s16 = tmp_path / f"{side}.ulc", tmp_path / f"{side}_f32.wav", tmp_path / f"{side}_16.wav"
        run_tool([os.path.join(REF_DIR, f"ulcencodetool_{side}"), str(wav), str(ulc), arg])
        run_tool([os.path.join(REF_DIR, f"ulcdecodetool_{side}"), str(ulc), str(f32), "-format:FLOAT32"])
        run_tool([os.path.join(REF_DIR, f"ulcdecodetool_{side}"), str(ulc), str(s16)])
        files[side] = [open(p, "rb").read() for p in (ulc, f32, s16)]
    for i, what in enumerate((".ulc", "float32 WAV", "PCM16 WAV")):
        assert len(files["amd"][i]) > 100
        assert files["amd"][i] == files["ref"][i], f"{what} written over libulc_amd.so differs from the real reference's"
