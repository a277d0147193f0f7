"""The case set of the full-reference pin (tests/test_oracle_fullref.py, tests/test_gpu_fullref.py,
tests/golden/make_fullref_digests.py) and the plumbing around oracle/_ref/ulc_ref_driver: the reference's seven libulc
sources compiled in place over the project's standin/Fourier.h (transforms = this project's spec v2), one stream per process.

Encoder cases are whole streams (PCM, BlockSize, channels, rate, mode, p0, p1); decoder cases are the encoder cases' streams
plus hand-assembled ones that only hold codes the format allocates (the reference does not bounds-check)."""
import hashlib
import os
import subprocess
import tempfile
import numpy as np
from ulc_testlib import ORACLE_DIR, synth_pcm, oracle_encode_debug, spec_stream
from refloop_cases import CASES as REFLOOP_CASES

REF_DIR = os.path.join(ORACLE_DIR, "_ref")
DRIVER = os.path.join(REF_DIR, "ulc_ref_driver")
FULL_SO = os.path.join(REF_DIR, "libulc_ref_full.so")
VBR, CBR, ABR = 0, 1, 2
SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
# every header code: overlap scale 0-7 x (no decimation, the 14 decimation patterns FormatSpecs.md allocates, 2h-Fh)
ALL_CODES = [s for s in range(8)] + [(p << 4) | 8 | s for p in range(2, 16) for s in range(8)]


def have_driver():
    return os.path.exists(DRIVER) and os.path.exists(FULL_SO)


def slot_for(bs, ch):
    return 2 * ch * bs + 16


def _q16(x):
    return np.ascontiguousarray(np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767) / 32768.0, dtype=np.float32)


# ---- encoder cases ----------------------------------------------------------------------------------------------------
def _refloop(tag):
    bs, ch, rate, nblk, sid, seed, mode, p0, p1 = REFLOOP_CASES[tag]
    return (synth_pcm(sid, nblk * bs, ch, rate, transient=True, seed=seed), bs, rate, mode, p0, p1)


def _ties(s, mode, p0):
    """test_encode_tie_straddle_uses_exact_heapsort_order's input: (L, R, L, R) - every key of channel 0 ties with channel 2."""
    base = synth_pcm(s, 12 * 512, 2, 44100, transient=True, seed=77)
    return (np.ascontiguousarray(np.concatenate([base, base], axis=1)), 512, 44100, mode, p0, 0.0)


def _degenerate(bs, ch, rate, which):
    """test_selection_bracket_on_degenerate_key_distributions' six signals (4 blocks)."""
    n = 4 * bs
    rng = np.random.default_rng(bs + ch)
    t = np.arange(n) / rate
    if which == 0:
        x = synth_pcm(1, n, ch, rate, transient=True, seed=5).copy(); x[:, -1] = 0.0                  # a silent channel
    elif which == 1:
        x = np.zeros((n, ch), np.float32); x[:, 0] = 0.4 * np.sin(2 * np.pi * 1000 * t) + 0.3 * np.sin(2 * np.pi * 5000 * t); x[:, -1] = x[:, 0]
    elif which == 2:
        x = np.zeros((n, ch), np.float32); x[bs // 3::bs, :] = 0.9                                       # an impulse per block
    elif which == 3:
        x = (synth_pcm(2, n, ch, rate, transient=False, seed=6) * np.float32(2.0 ** -14)).astype(np.float32)   # near silence
    elif which == 4:
        x = np.sign(np.sin(2 * np.pi * 440 * t)).astype(np.float32)[:, None].repeat(ch, 1) * np.float32(1.5)
    else:
        x = rng.uniform(-1, 1, (n, ch)).astype(np.float32)                                                # white noise
    return np.ascontiguousarray(np.round(x * 32768.0) / 32768.0, dtype=np.float32)


def _gaps(bs, ch, rate, nblk, seed):
    """Long stretches of digital silence between short tonal / noisy bursts inside each block: long zero runs (0h, 1h) and,
    at low quality, several noise runs (8h) and tails (Fh,Fh) per unit."""
    rng = np.random.default_rng(seed)
    n = nblk * bs
    t = np.arange(n) / rate
    x = np.zeros((n, ch))
    for c in range(ch):
        env = np.zeros(n)
        for _ in range(3 * nblk):
            p = int(rng.integers(0, n)); ln = int(rng.integers(bs // 16, bs // 4))
            env[p:p + ln] = rng.uniform(0.05, 0.5)
        tone = sum(rng.uniform(0.2, 0.5) * np.sin(2 * np.pi * rng.uniform(100, 0.45 * rate) * t) for _ in range(2))
        x[:, c] = env * (tone + rng.normal(0, 0.3, n))
    return _q16(x)


def _special(kind, bs, ch, nblk):
    n = nblk * bs
    x = np.zeros((n, ch), np.float32)
    if kind == "clip":                                            # full-scale square wave, beyond full scale before the grid
        x[:] = np.sign(np.sin(2 * np.pi * np.arange(n) / 97.0))[:, None] * 1.0
        x[x < 0] = -1.0; x[x > 0] = np.float32(32767 / 32768)
        return np.ascontiguousarray(x, np.float32)
    if kind == "dc":
        x[:] = np.float32(0.5)
        x[: bs // 2] = 0.0                                        # a step into DC: one transient, then nothing but DC
        return x
    if kind == "impulse":
        for k in range(nblk):
            x[k * bs + (37 * k + 11) % bs, k % ch] = np.float32(0.75)
        return x
    if kind == "denormal":                                        # denormal-level input (below FLT_MIN) and a few normal samples
        rng = np.random.default_rng(9)
        x[:] = (rng.integers(-1000, 1000, (n, ch)) * np.float32(2.0 ** -140)).astype(np.float32)
        x[n // 2, 0] = np.float32(2.0 ** -100)
        return x
    raise KeyError(kind)


def _shape(bs, ch):
    rate = {256: 22050, 512: 32000, 1024: 44100, 2048: 48000, 4096: 44100, 8192: 48000, 16384: 96000, 32768: 48000}[bs]
    nblk = max(3, min(8, 32768 * 3 // bs))
    return (synth_pcm(1000 + bs + ch, nblk * bs, ch, rate, transient=True, seed=bs * 7 + ch), bs, rate)


def _make_cases():
    cases = {}
    for tag in REFLOOP_CASES:
        cases["refloop_" + tag] = lambda tag=tag: _refloop(tag)
    for s in range(4):
        cases[f"ties_vbr50_s{s}"] = lambda s=s: _ties(s, VBR, 50.0)
        cases[f"ties_cbr96_s{s}"] = lambda s=s: _ties(s, CBR, 96.0)
    for bs, ch, rate in ((2048, 2, 44100), (4096, 2, 44100), (2048, 1, 48000), (1024, 2, 32000), (8192, 1, 44100)):
        for w in range(6):
            for mode, p0 in ((VBR, 100.0), (VBR, 50.0), (VBR, 1.0), (CBR, 96.0)):
                cases[f"degen_{bs}x{ch}_sig{w}_m{mode}_{p0:g}"] = lambda bs=bs, ch=ch, rate=rate, w=w, mode=mode, p0=p0: (
                    _degenerate(bs, ch, rate, w), bs, rate, mode, p0, 0.0)
    for bs, ch, nblk in ((2048, 2, 12), (32768, 1, 3)):
        for mode, p0 in ((VBR, 10.0), (VBR, 30.0), (CBR, 24.0)):
            cases[f"gaps_{bs}x{ch}_m{mode}_{p0:g}"] = lambda bs=bs, ch=ch, nblk=nblk, mode=mode, p0=p0: (
                _gaps(bs, ch, 44100, nblk, bs + ch), bs, 44100, mode, p0, 0.0)
    # the corner of test_rate_search_at_high_rates_over_several_calls: beyond full scale, ABR 229 kbps, 30 blocks
    for s in range(3):
        cases[f"highrate_abr229_s{s}"] = lambda s=s: (
            synth_pcm(s, 30 * 2048, 2, 48000, transient=True, seed=760153175) * np.float32(8.0), 2048, 48000, ABR, 228.95, 0.33)
    for kbps in (256.0, 320.0, 512.0):
        cases[f"highrate_cbr{kbps:g}"] = lambda kbps=kbps: (synth_pcm(7, 16 * 2048, 2, 48000, transient=True, seed=31), 2048, 48000, CBR, kbps, 0.0)
    for cplx in (0.02, 0.35, 0.98):
        cases[f"abr64_cplx{cplx:g}"] = lambda cplx=cplx: (synth_pcm(8, 16 * 2048, 2, 44100, transient=True, seed=32), 2048, 44100, ABR, 64.0, cplx)
    for q in (1.0, 100.0):
        for bs, ch in ((2048, 2), (256, 1), (8192, 2)):
            cases[f"vbr{q:g}_{bs}x{ch}"] = lambda q=q, bs=bs, ch=ch: (synth_pcm(9, 8 * bs, ch, 44100, transient=True, seed=33), bs, 44100, VBR, q, 0.0)
    for kind in ("clip", "dc", "impulse", "denormal"):
        for bs, ch, mode, p0 in ((2048, 2, VBR, 50.0), (512, 3, CBR, 128.0)):
            cases[f"{kind}_{bs}x{ch}_m{mode}"] = lambda kind=kind, bs=bs, ch=ch, mode=mode, p0=p0: (
                _special(kind, bs, ch, 6), bs, 44100, mode, p0, 0.0)
    for bs in SIZES:
        for i, ch in enumerate((1, 2, 3, 6)):
            mode, p0, p1 = ((VBR, 50.0, 0.0), (CBR, 96.0, 0.0), (ABR, 128.0, 0.4), (VBR, 70.0, 0.0))[i]
            cases[f"shape_{bs}x{ch}"] = lambda bs=bs, ch=ch, mode=mode, p0=p0, p1=p1: _shape(bs, ch) + (mode, p0, p1)
    # the geometry axis (tests/geometry_axis_testlib.py): the oracle's footing at the channel counts its cases add - gap sums at their
    # limit (16) and just behind it (17), 32, the header's last count (255) - and mono 4096 in a rate search; 9 blocks of 256 are more
    # samples than synth_pcm's delay of 7 per channel needs
    for ch in (16, 17, 32, 255):
        for mode, p0 in ((VBR, 50.0), (CBR, 48.0 * ((ch + 1) // 2))):
            cases[f"chan_256x{ch}_m{mode}_{p0:g}"] = lambda ch=ch, mode=mode, p0=p0: (
                synth_pcm(2000 + ch, 9 * 256, ch, 44100, transient=True, seed=256 * 7 + ch), 256, 44100, mode, p0, 0.0)
    cases["chan_4096x1_m1_64"] = lambda: (synth_pcm(2001, 6 * 4096, 1, 44100, transient=True, seed=4096 * 7 + 1), 4096, 44100, CBR, 64.0, 0.0)
    return cases


ENC_CASES = _make_cases()


def enc_case(tag):
    pcm, bs, rate, mode, p0, p1 = ENC_CASES[tag]()
    return np.ascontiguousarray(pcm, np.float32), bs, rate, mode, float(p0), float(p1)


# ---- decoder-only cases -----------------------------------------------------------------------------------------------
def _all_codes_stream(bs, ch, seed):
    rng = np.random.default_rng(seed)
    wc = [0, 0x3] + [int(c) for c in rng.permutation(ALL_CODES)]
    mid = len(wc) // 2
    wc[mid:mid] = [0x0, 0x0, 0x0]
    blocks, _, _ = spec_stream(wc, ch, bs, seed, silent_blocks=(mid, mid + 1, mid + 2))
    return blocks


def _opening_fh():
    """test_opening_Fh_quantizer_is_x86_shift_behaviour's block (a unit that opens with Fh: quantizer index -2), twice over."""
    nyb = [0x0, 0xF, 0x2, 0x9, 0x5, 0xF, 0x2, 0x3, 0xF, 0xE, 0xF]
    b = np.zeros(64, np.uint8)
    for i, v in enumerate(nyb):
        b[i // 2] |= v << (4 * (i & 1))
    return np.stack([b, b])


DEC_ONLY = {**{f"spec_{bs}x{ch}": (lambda bs=bs, ch=ch: (_all_codes_stream(bs, ch, bs + ch), bs, ch))
               for bs, ch in ((256, 6), (512, 3), (1024, 2), (2048, 1), (2048, 2), (4096, 6), (8192, 3), (16384, 2), (32768, 1))},
            "opening_Fh_256x1": lambda: (_opening_fh(), 256, 1)}


# ---- the driver -------------------------------------------------------------------------------------------------------
def driver_encode(pcm, bs, rate, mode, p0, p1, slot=None):
    n, ch = pcm.shape
    nblk = n // bs
    slot = slot or slot_for(bs, ch)
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.f32"), os.path.join(d, "out.bin")
        np.ascontiguousarray(pcm[:nblk * bs], np.float32).tofile(fi)
        subprocess.run([DRIVER, "enc", fi, fo, str(bs), str(ch), str(rate), str(mode), repr(float(np.float32(p0))),
                        repr(float(np.float32(p1))), str(nblk), str(slot)], check=True, timeout=600)
        rec = np.fromfile(fo, np.uint8).reshape(nblk, 16 + slot)
    hdr = np.ascontiguousarray(rec[:, :16]).view(np.int32)
    return dict(out=np.ascontiguousarray(rec[:, 16:]), bits=hdr[:, 0].copy(), wc=hdr[:, 1].copy(), nextwc=hdr[:, 2].copy(),
                cplx=hdr[:, 3].copy().view(np.float32))


def driver_decode(blocks, ch, bs):
    nblk, slot = blocks.shape
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.ascontiguousarray(blocks, np.uint8).tofile(fi)
        subprocess.run([DRIVER, "dec", fi, fo, str(bs), str(ch), str(nblk), str(slot)], check=True, timeout=600)
        raw = np.fromfile(fo, np.uint8)
    bits = raw[:4 * nblk].view(np.int32).copy()
    pcm = raw[4 * nblk:].view(np.float32).reshape(nblk * bs, ch).copy()
    return bits, pcm


def oracle_encode(pcm, bs, rate, mode, p0, p1, slot=None):
    return oracle_encode_debug(pcm, bs, rate, mode, p0, p1, slot=slot or slot_for(bs, pcm.shape[1]))


def payload(r):
    """The bytes a block really holds: (SizeBits+7)/8 of its slot."""
    return [r["out"][k, :(int(r["bits"][k]) + 7) // 8].tobytes() for k in range(len(r["bits"]))]


def enc_digest(r):
    h = hashlib.sha256()
    for p in payload(r):
        h.update(p)
    h.update(np.asarray(r["bits"], np.int32).tobytes()); h.update(np.asarray(r["wc"], np.int32).tobytes())
    h.update(np.asarray(r["cplx"], np.float32).tobytes())
    return h.hexdigest()


def dec_digest(bits, pcm):
    return hashlib.sha256(np.asarray(bits, np.int32).tobytes() + np.ascontiguousarray(pcm, np.float32).tobytes()).hexdigest()
