"""Low-rate crops (include/ulc_amd_lowrate.h) without a GPU: the referee's premise, the new header against the binding's second
table, ulcx_lowrate_block's arithmetic, the census of what the GPU cases' inputs hold, the refusals that need no device, and the
time alignment of the reduced stream against a band-limited decimation of the full decode."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import ulc_amd
import test_binding_signatures as B
import lowrate_testlib as LT
from ulc_testlib import same_bits

HEADER = os.path.join(ROOT, "include", "ulc_amd_lowrate.h")
BLOCK_SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
NAMES = ("ulcx_decode_crops_lowrate_dev", "ulcx_decode_crops_lowrate_dev_pcm16", "ulcx_decode_crops_lowrate_host",
         "ulcx_decode_crops_lowrate_ragged_dev", "ulcx_decode_crops_lowrate_ragged_dev_pcm16", "ulcx_decode_crops_lowrate_ragged_host")
ERR_ARG = -1


def _prototypes():
    """test_binding_signatures.prototypes() on the new header."""
    saved = B.HEADER
    B.HEADER = HEADER
    try:
        return B.prototypes()
    finally:
        B.HEADER = saved


PROTOS = _prototypes()


# ---------------------------------------------------------------------------------------------------------------------
# the referee's premise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted({n for n in LT.CASES}))
def test_at_ratio_one_the_referee_is_the_oracles_decoder(name):
    for f in LT.case_files(name):
        got = LT.referee_blocks(f.coef, f.wc, f.bs, 0)
        assert same_bits(got, f.pcm), f.name


# ---------------------------------------------------------------------------------------------------------------------
# header and table
# ---------------------------------------------------------------------------------------------------------------------
def test_the_new_header_and_the_second_table_name_the_same_functions():
    assert len(PROTOS) == 7
    assert set(PROTOS) == set(ulc_amd.EXT_EXPORTS) == set(ulc_amd.EXT_SIGNATURES)
    assert len(ulc_amd.EXT_EXPORTS) == len(set(ulc_amd.EXT_EXPORTS))
    assert not set(ulc_amd.EXT_EXPORTS) & set(ulc_amd.EXPORTS)
    for dev, twin in ulc_amd.EXT_PCM16_TWIN.items():
        assert dev in PROTOS and twin in PROTOS and "pcm16" in twin and "pcm16" not in dev, (dev, twin)
        assert ulc_amd.EXT_SIGNATURES[twin] == ulc_amd.EXT_SIGNATURES[dev], (dev, twin)
        assert len(PROTOS[twin][1]) == len(PROTOS[dev][1]), (dev, twin)
    assert sorted(ulc_amd.EXT_PCM16_TWIN.values()) == sorted(n for n in PROTOS if "pcm16" in n)
    assert '#include "ulc_amd.h"' in open(HEADER).read()


def test_every_new_entry_has_the_headers_arity_classes_return_and_element_types():
    typed = 0
    for name, (ret, params) in PROTOS.items():
        argtypes, restype = ulc_amd.EXT_SIGNATURES[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        assert ret in B.RETURNS and restype is B.RETURNS[ret], (name, ret)
        for k, (t, param) in enumerate(zip(argtypes, params)):
            if B.is_pointer(param):
                assert B.is_ctypes_pointer(t), (name, k, param, t)
                words = re.sub(r"\bconst\b|\*|\[\w*\]", " ", param).split()[:-1]
                if t not in (C.c_void_p, C.c_char_p) and len(words) == 1 and words[0] in B.ELEMENTS:
                    assert t._type_ is B.ELEMENTS[words[0]], (name, k, param, t)
                    typed += 1
            else:
                assert B.scalar_class(param) in B.SCALARS and t in B.SCALARS[B.scalar_class(param)], (name, k, param, t)
    assert typed >= 2 * sum(n.endswith("_host") for n in PROTOS), typed


def test_a_lowrate_entry_is_its_sample_crop_entry_with_lgd_behind_nsamples():
    for name in NAMES:
        twin = name.replace("lowrate", "samples")
        a, b = list(ulc_amd.EXT_SIGNATURES[name][0]), list(ulc_amd.SIGNATURES[twin][0])
        at = len(b) - (3 if "_dev" in name else 2)                # behind nSamples: in front of pcm, bits[, stream]
        assert a[:at] == b[:at] and a[at] is C.c_int and a[at + 1:] == b[at:], name
        pa, pb = PROTOS[name][1], B.PROTOS[twin][1]
        assert pa[:at] == pb[:at] and pa[at] == "int lgD" and pa[at + 1:] == pb[at:], name
        assert pa[at - 1] == "int nSamples"


def test_the_library_exports_and_the_python_layer_binds_them():
    import corpus
    import inspect
    l = ulc_amd.lib()
    for n in ulc_amd.EXT_EXPORTS:
        assert hasattr(l, n), n
    for m in ("decode_crops_lowrate", "decode_crops_lowrate_dev", "decode_crops_lowrate_ragged", "decode_crops_lowrate_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert inspect.signature(corpus.CropCorpus.sample_crops).parameters["lowrate"].default == 0


# ---------------------------------------------------------------------------------------------------------------------
# ulcx_lowrate_block
# ---------------------------------------------------------------------------------------------------------------------
def test_lowrate_block_arithmetic():
    l = ulc_amd.lib()
    for bs in BLOCK_SIZES:
        for lg in range(-1, 5):
            want = bs >> lg if 0 <= lg <= 3 and (bs >> lg) >= 256 else 0
            assert l.ulcx_lowrate_block(bs, lg) == want == ulc_amd.lowrate_block(bs, lg), (bs, lg)
    for bs in (0, -2048, 128, 1000, 3000, 65536):              # no BlockSize at all
        for lg in range(0, 4):
            assert l.ulcx_lowrate_block(bs, lg) == 0, (bs, lg)


def test_refusals_without_a_device():
    """No object: lgD outside 0 .. 3 is refused first, under the entry's own name; then what the sample-crop entry refuses."""
    l = C.CDLL(ulc_amd.LIB_PATH)                                # (a handle of its own: every pointer a plain address)
    l.ulcx_last_error.restype = C.c_char_p
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    P, I, LL = C.c_void_p, C.c_int, C.c_longlong
    strided = [P, I, P, LL, P, P, I, P, I, P, P, P, I, I, P, P]
    ragged = [P, I, P, LL, P, P, LL, P, P, I, P, P, P, I, I, P, P]
    for name in NAMES:
        fn = getattr(l, name)
        is_ragged, is_dev = "ragged" in name, "_dev" in name
        fn.argtypes = (ragged if is_ragged else strided) + ([P] if is_dev else [])
        fn.restype = I
        head = [None, 1, p, 1, p, p, 1, p, p] if is_ragged else [None, 1, p, 1, p, p, 1, p]
        tail = [p, p] + ([None] if is_dev else [])
        for lg in (-1, 4, 17):
            assert fn(*head, 1, p, p, p, 5, lg, *tail) == ERR_ARG
            msg = l.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and f"lgD {lg}" in msg, msg
        for lg in (0, 1, 3):
            assert fn(*head, 1, p, p, p, 0, lg, *tail) == ERR_ARG
            assert "nSamples 0" in l.ulcx_last_error().decode()
            assert fn(*head, 1, p, p, None, 5, lg, *tail) == ERR_ARG
            assert l.ulcx_last_error().decode() == name + ": no decoder"


# ---------------------------------------------------------------------------------------------------------------------
# the census of the GPU cases' inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LT.CASES))
def test_census_of_a_gpu_cases_inputs(name):
    from test_transform_referee import ALL_CODES
    bs, ch, lgD = LT.CASES[name]
    cz = LT.census(name)
    print(name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in cz.items()})
    assert cz["plain_cross"] > 0 and cz["run_cross"] > 0 and cz["tail_cross"] > 0, (name, cz)
    if bs >= 4096:
        assert cz["draws_max"] > 2048, (name, cz["draws_max"])
    if name.startswith("codes"):
        assert cz["codes"] == set(ALL_CODES), (name, cz["codes"])
    lc = LT.low_case(name)                                     # the dead block: the killed copy ends at it by the oracle's model
    st = LT.D.Stream(lc.cor.files[0])
    assert st.model(lc.killed, lc.dead_at, 2)[2] == 0 and st.model(lc.killed, lc.dead_at - 1, 1)[2] == 1, name
    assert 1 <= lc.dead_at <= lc.cor.K[0] - 2


def test_every_header_code_is_covered_by_the_code_cases():
    from test_transform_referee import ALL_CODES
    for name in LT.CASES:
        if name.startswith("codes"):
            f = LT.case_files(name)[0]
            assert {int(w) if w & 8 else int(w) & 7 for w in f.wc} == set(ALL_CODES), name


# ---------------------------------------------------------------------------------------------------------------------
# alignment: reduced sample m sits at full-rate time D m + (D - 1) / 2
# ---------------------------------------------------------------------------------------------------------------------
def _brickwall(x, D, offset):
    """x [n] sampled at D m + offset behind an FFT brick wall at fs / 2D (periodic extension: the edges are cut off by the caller)."""
    n = x.size
    X = np.fft.rfft(x.astype(np.float64))
    k = np.arange(X.size)
    X[n // (2 * D):] = 0
    return np.fft.irfft(X * np.exp(2j * np.pi * k * offset / n), n)[::D]      # the band-limited signal moved left by `offset`, every D-th sample


def _snr(ref, got):
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((ref - got) ** 2))


def test_the_reduced_stream_is_aligned_at_half_a_decimation_step():
    from ulc_testlib import oracle_encode_debug, oracle_decode_stream_coefs, wc_of
    bs, ch, K, rate = 1024, 1, 12, 44100
    t = np.arange(K * bs)
    pcm = sum(a * np.sin(2 * np.pi * f * t / rate + p) for a, f, p in ((0.3, 220.0, 0.1), (0.2, 997.0, 1.3), (0.1, 1710.0, 2.2)))
    pcm = pcm.astype(np.float32).reshape(-1, 1)
    r = oracle_encode_debug(pcm, bs, rate, 0, 80.0, slot=2 * ch * bs + 16)
    rc, full, obits, coefs = oracle_decode_stream_coefs(r["out"], ch, bs)
    assert rc == 0
    wc = wc_of(r["out"])
    full = full.reshape(-1)
    lines = []
    for lgD in (1, 2, 3):
        D = 1 << lgD
        low = LT.referee_blocks(coefs.reshape(K, ch, bs), wc, bs, lgD).reshape(-1).astype(np.float64)
        mid = (D - 1) / 2
        cut = slice(2 * bs // D, (K - 2) * bs // D)             # away from the stream's ends and the brick wall's wrap
        snr = {off: _snr(_brickwall(full, D, off)[cut], low[cut]) for off in (mid - 0.5, mid, mid + 0.5)}
        lines.append(f"D = {D}: SNR against the brick-wall decimation at offsets {mid - 0.5:g} / {mid:g} / {mid + 0.5:g}: "
                     + " / ".join(f"{snr[o]:.1f}" for o in sorted(snr)) + " dB")
        print(lines[-1])
        assert snr[mid] > snr[mid - 0.5] and snr[mid] > snr[mid + 0.5], (D, snr)
    out = os.environ.get("ULCX_LOWRATE_QUALITY_OUT")           # (set to profiles/lowrate_quality.txt to rewrite that file's figures)
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
