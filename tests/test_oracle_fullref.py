"""The oracle against the REAL reference, whole: all seven libulc sources (ulcEncoder.c, ulcEncoder_BlockTransform.c,
ulcEncoder_Encode.c, ulcEncoder_WindowControl.c, ulcEncoder_Psyopt.c, ulcEncoder_NoiseFill.c, ulcDecoder.c) compiled in place
over the project's standin/Fourier.h into oracle/_ref/libulc_ref_full.so, driven one stream per process by
oracle/_ref/ulc_ref_driver.  The stand-in forwards the two transforms to orc_fourier.c (fourier spec v2, refereed in float64
by test_transform_referee.py), so this pins everything else: the rate-control drivers, the lapping FIFO, M/S, the keys,
BlockComplexity and the sort, the quantiser zones, noise runs and tails, the nybble writer, the rate search and the decoder.

  * where the full build exists: the oracle writes byte-equal blocks with equal sizes, WindowCtrl and BlockComplexity on every
    encoder case of fullref_cases.py, its decoder's PCM is bit-equal to the real decoder's on every stream, and the build
    reproduces the committed digests (so they cannot go stale);
  * everywhere: the oracle's streams and PCM equal the digests the full build produced (tests/golden/fullref_digests.json,
    made by tests/golden/make_fullref_digests.py), and the case set reaches what it claims (coverage test)."""
import functools
import json
import os
import numpy as np
import pytest
from fullref_cases import (ENC_CASES, DEC_ONLY, CBR, enc_case, have_driver, driver_encode, driver_decode, oracle_encode,
                           payload, enc_digest, dec_digest, slot_for, FULL_SO)
from ulc_testlib import oracle_decode_stream
from spec_decoder import decode_block_coefficients

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "fullref_digests.json")))
needs_ref = pytest.mark.skipif(not have_driver(), reason="oracle/_ref/libulc_ref_full.so not built (reference tree absent at build time)")
COMPARED = {"streams": 0, "blocks": 0, "decoder streams": 0, "decoder blocks": 0}


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    yield
    if COMPARED["streams"] or COMPARED["decoder streams"]:
        tr = request.config.pluginmanager.get_plugin("terminalreporter")
        line = "fullref: compared with the real reference: %(streams)d encoder streams / %(blocks)d blocks, " \
               "%(decoder streams)d decoder streams / %(decoder blocks)d blocks" % COMPARED
        if tr is not None:
            tr.write_line(line)
        else:
            print(line)


@functools.lru_cache(maxsize=None)
def _oracle(tag):
    """The oracle's encode of a case (sizes, WindowCtrl, BlockComplexity, bytes, tie-straddle flags) and its decode."""
    pcm, bs, rate, mode, p0, p1 = enc_case(tag)
    r = oracle_encode(pcm, bs, rate, mode, p0, p1)
    n = r["keys"].shape[1]
    ties = []
    for k in range(len(r["bits"])):
        nout = int(r["nout"][k])
        if 0 < nout < n:
            by_rank = np.empty(n, np.float32); by_rank[r["ranks"][k]] = r["keys"][k]
            ties.append(bool(by_rank[nout - 1] == by_rank[nout]) and bool(np.isfinite(by_rank[nout])))
        else:
            ties.append(False)
    rc, dpcm, dbits = oracle_decode_stream(r["out"], pcm.shape[1], bs)
    assert rc == 0
    return dict(out=r["out"], bits=r["bits"], wc=r["wc"], cplx=r["cplx"], ties=np.array(ties), dbits=dbits, dpcm=dpcm,
                shape=(bs, pcm.shape[1], rate, mode, p0, p1))


def test_committed_digests_cover_the_case_set():
    assert set(GOLD["encode"]) == set(ENC_CASES), "tests/golden/fullref_digests.json is out of step with fullref_cases.py"
    assert set(GOLD["decode_only"]) == set(DEC_ONLY)


@pytest.mark.parametrize("tag", sorted(ENC_CASES))
def test_oracle_equals_committed_real_reference_digests(tag):
    r = _oracle(tag)
    g = GOLD["encode"][tag]
    assert len(r["bits"]) == g["blocks"] and sum(len(p) for p in payload(r)) == g["bytes"]
    assert enc_digest(r) == g["stream_sha256"], "the oracle's stream differs from the one the real reference wrote"
    assert dec_digest(r["dbits"], r["dpcm"]) == g["decode_sha256"], "the oracle's decode differs from the real decoder's"


@pytest.mark.parametrize("tag", sorted(DEC_ONLY))
def test_oracle_decoder_equals_committed_real_decoder_digests_on_assembled_streams(tag):
    blocks, bs, ch = DEC_ONLY[tag]()
    rc, pcm, bits = oracle_decode_stream(blocks, ch, bs)
    assert rc == 0
    assert dec_digest(bits, pcm) == GOLD["decode_only"][tag]["decode_sha256"]


@needs_ref
def test_the_full_build_is_what_it_says():
    import ctypes as C
    lib = C.CDLL(FULL_SO)
    for s in ("ULC_EncoderState_Init", "ULC_EncoderState_Destroy", "ULC_EncodeBlock_CBR", "ULC_EncodeBlock_ABR",
              "ULC_EncodeBlock_VBR", "ULC_DecoderState_Init", "ULC_DecoderState_Destroy", "ULC_DecodeBlock",
              "Fourier_MDCT_MDST", "Fourier_IMDCT", "orc_mdct_mdst", "orc_imdct"):
        assert hasattr(lib, s), s


@needs_ref
@pytest.mark.parametrize("tag", sorted(ENC_CASES))
def test_oracle_encoder_and_decoder_equal_the_real_reference(tag):
    pcm, bs, rate, mode, p0, p1 = enc_case(tag)
    ch = pcm.shape[1]
    a = driver_encode(pcm, bs, rate, mode, p0, p1)
    b = _oracle(tag)
    for k in range(len(a["bits"])):
        assert a["wc"][k] == b["wc"][k], f"block {k}: WindowCtrl {b['wc'][k]:#x}, real {a['wc'][k]:#x}"
        assert a["cplx"][k].tobytes() == b["cplx"][k].tobytes(), f"block {k}: BlockComplexity {b['cplx'][k]}, real {a['cplx'][k]}"
        assert a["bits"][k] == b["bits"][k], f"block {k}: size {b['bits'][k]}, real {a['bits'][k]}"
    assert payload(a) == payload(b), [k for k, (x, y) in enumerate(zip(payload(a), payload(b))) if x != y]
    assert np.array_equal(a["nextwc"][:-1], a["wc"][1:]), "NextWindowCtrl is not the next block's WindowCtrl"
    g = GOLD["encode"][tag]
    assert enc_digest(a) == g["stream_sha256"], "the full build no longer writes the committed stream: regenerate the digests"
    COMPARED["streams"] += 1; COMPARED["blocks"] += len(a["bits"])
    bits, dpcm = driver_decode(a["out"], ch, bs)
    assert np.array_equal(bits, b["dbits"]), "bits read differ from the real decoder's"
    assert dpcm.view(np.uint32).tobytes() == b["dpcm"].view(np.uint32).tobytes(), "decoded PCM differs from the real decoder's"
    assert dec_digest(bits, dpcm) == g["decode_sha256"]
    COMPARED["decoder streams"] += 1; COMPARED["decoder blocks"] += len(bits)


@needs_ref
@pytest.mark.parametrize("tag", sorted(DEC_ONLY))
def test_oracle_decoder_equals_the_real_decoder_on_assembled_streams(tag):
    """Hand-assembled streams: every one of the 120 header codes and every code the format allocates, and the opening-Fh
    unit whose quantizer is the reference binary's negative shift (quantizer 0.0 on x86-64)."""
    blocks, bs, ch = DEC_ONLY[tag]()
    bits, pcm = driver_decode(blocks, ch, bs)
    rc, opcm, obits = oracle_decode_stream(blocks, ch, bs)
    assert rc == 0 and np.array_equal(bits, obits)
    assert pcm.view(np.uint32).tobytes() == opcm.view(np.uint32).tobytes(), "decoded PCM differs from the real decoder's"
    assert dec_digest(bits, pcm) == GOLD["decode_only"][tag]["decode_sha256"]
    COMPARED["decoder streams"] += 1; COMPARED["decoder blocks"] += len(bits)


def test_case_set_reaches_what_it_claims():
    """Counted over the oracle's streams (equal to the real reference's by the digest tests) with the spec decoder."""
    kinds, headers, ties, tight = {}, set(), 0, 0
    for tag in ENC_CASES:
        r = _oracle(tag)
        bs, ch, rate, mode, p0, p1 = r["shape"]
        for k in range(len(r["bits"])):
            nb = (int(r["bits"][k]) + 7) // 8
            blk = np.zeros(nb + 8, np.uint8); blk[:nb] = r["out"][k, :nb]
            _, _, pos = decode_block_coefficients(blk, ch, bs, kinds)
            assert 4 * pos == r["bits"][k] or 4 * pos + 4 == r["bits"][k], (tag, k)
            w = int(r["wc"][k])
            if w & 8:
                headers.add(w >> 4 & 15)
            if mode == CBR:
                budget = int(np.float32(np.float32(bs) * np.float32(p0)) * np.float32(1000.0) / np.float32(rate))
                assert r["bits"][k] <= budget, (tag, k)
                tight += budget - int(r["bits"][k]) < 8
        ties += int(r["ties"].sum())
    for k in ("zero_run", "long_zero_run", "noise_run", "tail", "quantizer", "ext_quantizer", "stop", "coefficient"):
        assert kinds.get(k, 0) > 0, (k, kinds)
    assert kinds["noise_run"] > 100 and kinds["tail"] > 10, kinds
    assert len(headers) >= 6, sorted(headers)
    assert ties >= 1, "no block has its threshold tie group straddling the cut"
    assert tight >= 1, "no CBR block lands within a byte of its budget"
    print(f"codes {kinds}; decimation patterns {sorted(headers)}; tie-straddle blocks {ties}; CBR blocks within a byte {tight}")
