"""Mid and side crops (include/ulc_amd_part.h) without a GPU: the new header against the binding's third table, ulcx_part_channels'
arithmetic, the refusals that need no device, the definition tied to the oracle at lgD 0, the census of what the GPU cases' inputs
hold, and how far the coded mid may lie from the folded stereo decode.

The cases (part_testlib.CASES): 256x2/0, 1024x2/1, 2048x2/0, 2048x2/1, 2048x2/3, 4096x2/0, 4096x2/1, 8192x2/1, 8192x2/0, 512x1/0,
2048x3/1, 1024x6/2, codes 2048x2/1, codes 1024x1/0."""
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
import part_testlib as PT
from ulc_testlib import same_bits

HEADER = os.path.join(ROOT, "include", "ulc_amd_part.h")
NAMES = ("ulcx_decode_crops_part_dev", "ulcx_decode_crops_part_dev_pcm16", "ulcx_decode_crops_part_host",
         "ulcx_decode_crops_part_ragged_dev", "ulcx_decode_crops_part_ragged_dev_pcm16", "ulcx_decode_crops_part_ragged_host")
ERR_ARG = -1


def _prototypes(header):
    """test_binding_signatures.prototypes() on another header."""
    saved = B.HEADER
    B.HEADER = header
    try:
        return B.prototypes()
    finally:
        B.HEADER = saved


PROTOS = _prototypes(HEADER)
LOW_PROTOS = _prototypes(os.path.join(ROOT, "include", "ulc_amd_lowrate.h"))


# ---------------------------------------------------------------------------------------------------------------------
# header and table
# ---------------------------------------------------------------------------------------------------------------------
def test_the_new_header_and_the_third_table_name_the_same_functions():
    assert len(PROTOS) == 7 and set(NAMES) | {"ulcx_part_channels"} == set(PROTOS)
    assert set(PROTOS) == set(ulc_amd.PART_EXPORTS) == set(ulc_amd.PART_SIGNATURES)
    assert len(ulc_amd.PART_EXPORTS) == len(set(ulc_amd.PART_EXPORTS))
    for dev, twin in ulc_amd.PART_PCM16_TWIN.items():
        assert dev in PROTOS and twin in PROTOS and "pcm16" in twin and "pcm16" not in dev, (dev, twin)
        assert ulc_amd.PART_SIGNATURES[twin] == ulc_amd.PART_SIGNATURES[dev], (dev, twin)
        assert len(PROTOS[twin][1]) == len(PROTOS[dev][1]), (dev, twin)
    assert sorted(ulc_amd.PART_PCM16_TWIN.values()) == sorted(n for n in PROTOS if "pcm16" in n)
    text = open(HEADER).read()
    assert '#include "ulc_amd_lowrate.h"' in text
    assert re.search(r"#define\s+ULCX_PART_MID\s+0\b", text) and re.search(r"#define\s+ULCX_PART_SIDE\s+1\b", text)
    assert (ulc_amd.PART_MID, ulc_amd.PART_SIDE) == (0, 1)


def test_the_three_tables_are_disjoint_and_the_first_two_keep_their_size():
    a, b, c = set(ulc_amd.SIGNATURES), set(ulc_amd.EXT_SIGNATURES), set(ulc_amd.PART_SIGNATURES)
    assert not a & b and not a & c and not b & c
    assert len(b) == len(LOW_PROTOS) == 7                      # the second table: the low-rate header's entries and nothing else
    assert len(a) == len(B.PROTOS)                             # the first: ulc_amd.h's
    assert not any("part" in n for n in a | b)


def test_every_new_entry_has_the_headers_arity_classes_return_and_element_types():
    typed = 0
    for name, (ret, params) in PROTOS.items():
        argtypes, restype = ulc_amd.PART_SIGNATURES[name]
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


def test_a_part_entry_is_its_lowrate_entry_with_part_behind_lgd():
    for name in NAMES:
        twin = name.replace("part", "lowrate")
        a, b = list(ulc_amd.PART_SIGNATURES[name][0]), list(ulc_amd.EXT_SIGNATURES[twin][0])
        at = len(b) - (3 if "_dev" in name else 2)                # behind lgD: in front of pcm, bits[, stream]
        assert a[:at] == b[:at] and a[at] is C.c_int and a[at + 1:] == b[at:], name
        pa, pb = PROTOS[name][1], LOW_PROTOS[twin][1]
        assert pa[:at] == pb[:at] and pa[at] == "int part" and pa[at + 1:] == pb[at:], name
        assert pa[at - 1] == "int lgD" and pa[at - 2] == "int nSamples"


def test_the_library_exports_and_the_python_layer_binds_them():
    import corpus
    import inspect
    l = ulc_amd.lib()
    for n in ulc_amd.PART_EXPORTS:
        assert hasattr(l, n), n
    for m in ("decode_crops_part", "decode_crops_part_dev", "decode_crops_part_ragged", "decode_crops_part_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert inspect.signature(corpus.CropCorpus.sample_crops).parameters["part"].default is None


# ---------------------------------------------------------------------------------------------------------------------
# ulcx_part_channels; refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_part_channels_arithmetic():
    l = ulc_amd.lib()
    for ch in range(1, 256):
        for part in range(-1, 3):
            want = (ch + 1 - part) // 2 if part in (0, 1) else 0
            assert l.ulcx_part_channels(ch, part) == want == ulc_amd.part_channels(ch, part) == PT.part_channels(ch, part), (ch, part)
        assert l.ulcx_part_channels(ch, 0) + l.ulcx_part_channels(ch, 1) == ch
    assert l.ulcx_part_channels(1, 1) == 0 and l.ulcx_part_channels(3, 0) == 2 and l.ulcx_part_channels(3, 1) == 1
    for ch in (0, -1, 256):
        assert l.ulcx_part_channels(ch, 0) == 0 and l.ulcx_part_channels(ch, 1) == 0


def test_refusals_without_a_device():
    """No object: part outside 0 .. 1 is refused first, then lgD outside 0 .. 3, each under the entry's own name; then what the
    low-rate entry refuses.  (The side of a mono corpus needs an object: tests/test_gpu_part.py.)"""
    l = C.CDLL(ulc_amd.LIB_PATH)                                # (a handle of its own: every pointer a plain address)
    l.ulcx_last_error.restype = C.c_char_p
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    P, I, LL = C.c_void_p, C.c_int, C.c_longlong
    strided = [P, I, P, LL, P, P, I, P, I, P, P, P, I, I, I, P, P]
    ragged = [P, I, P, LL, P, P, LL, P, P, I, P, P, P, I, I, I, P, P]
    for name in NAMES:
        fn = getattr(l, name)
        is_ragged, is_dev = "ragged" in name, "_dev" in name
        fn.argtypes = (ragged if is_ragged else strided) + ([P] if is_dev else [])
        fn.restype = I
        head = [None, 1, p, 1, p, p, 1, p, p] if is_ragged else [None, 1, p, 1, p, p, 1, p]
        tail = [p, p] + ([None] if is_dev else [])
        for part in (-1, 2, 17):
            for lg in (0, 9):                                   # (a bad part is named whatever lgD is)
                assert fn(*head, 1, p, p, p, 5, lg, part, *tail) == ERR_ARG
                msg = l.ulcx_last_error().decode()
                assert msg.startswith(name + ":") and f"part {part}" in msg, msg
        for part in (0, 1):
            for lg in (-1, 4):
                assert fn(*head, 1, p, p, p, 5, lg, part, *tail) == ERR_ARG
                msg = l.ulcx_last_error().decode()
                assert msg.startswith(name + ":") and f"lgD {lg}" in msg, msg
            for lg in (0, 3):
                assert fn(*head, 1, p, p, p, 0, lg, part, *tail) == ERR_ARG
                assert "nSamples 0" in l.ulcx_last_error().decode()
                assert fn(*head, 1, p, p, None, 5, lg, part, *tail) == ERR_ARG
                assert l.ulcx_last_error().decode() == name + ": no decoder"


# ---------------------------------------------------------------------------------------------------------------------
# the definition, tied to the oracle at lgD 0
# ---------------------------------------------------------------------------------------------------------------------
def _geometry_cases():
    """One case per set of files."""
    seen, out = set(), []
    for name, (bs, ch, _, codes) in PT.CASES.items():
        if (bs, ch, codes) not in seen:
            seen.add((bs, ch, codes)); out.append(name)
    return out


@pytest.mark.parametrize("name", _geometry_cases())
def test_the_per_channel_planes_unmixed_are_the_oracles_decode(name):
    """What the one-channel referee holds for channels 2 j and 2 j + 1, un-mixed in float32 as a + b, a - b (ulcDecoder.c:281-289), is
    File.pcm bit for bit; an unpaired last channel, and a mono file's one channel, is File.pcm as it stands."""
    for f in PT.case_files(name):
        planes = [PT.channel_plane(f, 0, c) for c in range(f.ch)]            # [K][bs] each
        got = np.zeros_like(f.pcm)
        for c in range(0, f.ch - 1, 2):
            got[:, :, c], got[:, :, c + 1] = planes[c] + planes[c + 1], planes[c] - planes[c + 1]
        if f.ch & 1:
            got[:, :, f.ch - 1] = planes[f.ch - 1]
        assert got.dtype == np.float32 and same_bits(got, f.pcm), f.name


# ---------------------------------------------------------------------------------------------------------------------
# the census of the GPU cases' inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PT.CASES))
def test_census_of_a_gpu_cases_inputs(name):
    """Every case has un-decimated and decimated blocks, a silent block, a row that starts in the block behind a decimated one and -
    where it has a side channel at all, i.e. not the mono cases - a block whose side channel draws noise behind a mid channel that
    drew noise, so that a side state taken from the block's start shows."""
    bs, ch, lgD, codes = PT.CASES[name]
    cz = PT.census(name)
    print(name, cz)
    assert cz["whole"] > 0 and cz["decimated"] > 0 and cz["silent"] > 0 and cz["behind_decimated"] > 0, (name, cz)
    if ch > 1:
        assert cz["side_after_mid"] > 0, (name, cz)
    pc = PT.part_case(name)
    table = pc.row_table(3 * pc.bsr + 1)
    assert 20 <= len(table) <= 30
    starts_behind = [(f, s) for f, s, _ in table if 0 <= f < pc.cor.F - 1 and s >= pc.bsr and s // pc.bsr < pc.cor.K[f]
                     and PT.decimated(pc.cor.files[f], s // pc.bsr - 1)]
    assert starts_behind, name
    assert len({f for f, _, _ in table}) < len(table)                       # a file named twice
    assert any(s % pc.bsr == 0 and s > 0 for _, s, _ in table) and any(s % pc.bsr == 1 for _, s, _ in table)
    assert any(s % pc.bsr == pc.bsr - 1 for _, s, _ in table) and any(l is not None and 0 < l < 3 * pc.bsr + 1 for _, _, l in table)
    assert any(f < 0 for f, _, _ in table) and any(f >= pc.cor.F for f, _, _ in table) and any(s < 0 for _, s, _ in table)
    z, d = pc.cor.F - 1, pc.dead_at
    assert (z, (d + 1) * pc.bsr, 3 * pc.bsr + 1) in table and any(f == z and s // pc.bsr > d + 1 for f, s, _ in table)
    if codes:
        from test_transform_referee import ALL_CODES
        f = PT.case_files(name)[0]
        assert {int(w) if w & 8 else int(w) & 7 for w in f.wc} == set(ALL_CODES), name
    st = PT.D.Stream(pc.cor.files[0])                          # the dead block: the killed copy ends at it by the oracle's model
    killed = pc.cor.payloads[z]
    assert st.model(killed, d, 2)[2] == 0 and st.model(killed, d - 1, 1)[2] == 1, name
    assert 1 <= d <= pc.cor.K[0] - 2


# ---------------------------------------------------------------------------------------------------------------------
# the coded mid against the folded stereo decode
# ---------------------------------------------------------------------------------------------------------------------
def _exact(x):
    """float32 array -> Python integers (object array): x * 2^202, exactly (a float32 is an integer below 2^53 times 2^(e - 53), e >= -148)."""
    m, e = np.frexp(np.asarray(x, np.float32).astype(np.float64).reshape(-1))
    return (m * 2.0 ** 53).astype(np.int64).astype(object) * (2 ** (e.astype(np.int64).astype(object) + 149))


@pytest.mark.parametrize("name", [n for n in _geometry_cases() if PT.CASES[n][1] > 1])
def test_mid_is_the_folded_stereo_decode_up_to_the_unmixs_two_roundings(name):
    """a, b: the mid and side planes (float32).  The decoder's un-mix forms L = fl(a + b) = (a + b)(1 + e1) and R = fl(a - b) =
    (a - b)(1 + e2) with |e1|, |e2| <= u = 2^-24 (round to nearest; no underflow term: a float32 sum that is subnormal is exact).
    Folded without further rounding,
        (L + R) / 2 = a + ((a + b) e1 + (a - b) e2) / 2,   so   |(L + R) / 2 - a| <= u (|a + b| + |a - b|) / 2 = u max(|a|, |b|),
    and likewise |(L - R) / 2 - b| <= u max(|a|, |b|).  The test asserts exactly these bounds, sample by sample, in integer
    arithmetic (every float32 as an integer multiple of 2^-202: no rounding of the test's own): |L + R - 2 a| 2^23 <= max(|a|, |b|).
    It also asserts that the bound is not idle: somewhere the coded mid and the fold do differ."""
    differs = 0
    for f in PT.case_files(name):
        for c in range(0, f.ch - 1, 2):
            a, b = _exact(PT.channel_plane(f, 0, c)), _exact(PT.channel_plane(f, 0, c + 1))
            L, R = _exact(f.pcm[:, :, c]), _exact(f.pcm[:, :, c + 1])
            bound = np.maximum(np.abs(a), np.abs(b))
            em, es = np.abs(L + R - 2 * a) * 2 ** 23, np.abs(L - R - 2 * b) * 2 ** 23
            worst = max((float(x) / float(y) for x, y in zip(em, bound) if y), default=0.0)
            print(f.name, "pair", c, "largest |mid - fold| / (u max(|a|, |b|)):", worst)
            assert (em <= bound).all() and (es <= bound).all(), (f.name, c)
            differs += int((em > 0).sum())
    assert differs > 0, name
