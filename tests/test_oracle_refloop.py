"""The real reference functions INSIDE a whole-stream oracle encode (round-5 verdict item 3).

oracle/_ref/liboracle_refloop.so is this restatement with ULCi_GetWindowCtrl, ULCi_CalculateNoiseLogSpectrum,
ULCi_CalculatePsychoacoustics, ULCi_GetNoiseQ and ULCi_GetHFExtParams - compiled in place from /root/reference - called at
the reference's own call sites (ulcEncoder_BlockTransform.c:115,286,329; ulcEncoder_Encode.c:153,284) with the same
pointers and aliasing.  Two checks:
  * where that library exists: it and the pure restatement write byte-equal streams (sizes, WindowCtrl, BlockComplexity)
    for every case, and the digests of what entered and left each of the five functions agree call for call;
  * everywhere (also on the GPU box, where the reference is absent): the pure restatement's digests and streams equal the
    committed ones the refloop build produced (tests/golden/refloop_digests.json, made by make_refloop_digests.py).
This moves those five functions from "equal on synthetic inputs" (test_oracle_pinned.py) to "equal on every input the
configurations feed them, in situ".  ulcEncoder.c, ulcEncoder_BlockTransform.c, ulcEncoder_Encode.c and ulcDecoder.c (each
includes Fourier.h of the absent libfourier) are pinned separately, by the full reference build over the project's
standin/Fourier.h (tests/test_oracle_fullref.py)."""
import json
import os
import numpy as np
import pytest
from refloop_cases import CASES, SITES, run_case, load_refloop, load_pure

HERE = os.path.dirname(os.path.abspath(__file__))
REFLOOP = load_refloop()
GOLD = json.load(open(os.path.join(HERE, "golden", "refloop_digests.json")))


def test_the_two_builds_are_what_they_say():
    assert load_pure().orc_site_is_refloop() == 0
    if REFLOOP is not None:
        assert REFLOOP.orc_site_is_refloop() == 1


@pytest.mark.parametrize("tag", sorted(CASES))
def test_restatement_equals_committed_real_function_digests(tag):
    r = run_case(load_pure(), tag)
    g = GOLD[tag]
    assert r["cnt"] == g["calls"], "the five functions were called a different number of times"
    for s in SITES:
        assert "%016x" % r["dig"][s] == g["sites"][s], f"{s}: what entered / left the restated function differs from the real one's"
    assert r["sha"] == g["stream_sha256"]
    # every site is exercised by the case set as a whole; the noise-fill ones by this case unless it is tiny
    assert r["cnt"]["GetWindowCtrl"] == r["blocks"] and r["cnt"]["CalculatePsychoacoustics"] == r["blocks"]
    assert r["cnt"]["CalculateNoiseLogSpectrum"] >= r["blocks"] * CASES[tag][1]


def test_case_set_reaches_every_site_and_decimated_blocks():
    tot = {s: sum(GOLD[t]["calls"][s] for t in GOLD) for s in SITES}
    assert all(v > 0 for v in tot.values()), tot
    assert tot["GetNoiseQ"] > 1000 and tot["GetHFExtParams"] > 100, tot
    # decimated blocks call the noise spectrum once per subblock: more calls than (block, channel) pairs somewhere
    assert any(GOLD[t]["calls"]["CalculateNoiseLogSpectrum"] > GOLD[t]["blocks"] * CASES[t][1] for t in GOLD)


@pytest.mark.skipif(REFLOOP is None, reason="oracle/_ref/liboracle_refloop.so not built (/root/reference absent)")
@pytest.mark.parametrize("tag", sorted(CASES))
def test_real_functions_in_the_loop_write_the_same_stream(tag):
    a = run_case(load_pure(), tag)
    b = run_case(REFLOOP, tag)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["wc"], b["wc"])
    assert a["cplx"].tobytes() == b["cplx"].tobytes()
    assert a["out"].tobytes() == b["out"].tobytes()
    assert a["cnt"] == b["cnt"] and a["dig"] == b["dig"]
