#!/usr/bin/env python3
"""Generates tests/golden/fullref_digests.json.  Run where oracle/_ref/ulc_ref_driver exists (oracle/Makefile builds it, with
_ref/libulc_ref_full.so, only where the reference tree is present).

For every encoder case of tests/fullref_cases.py the real reference - all seven libulc sources over the project's
standin/Fourier.h - encodes the stream; recorded are the sha256 of its blocks, sizes, WindowCtrl and BlockComplexity, and the
sha256 of the real decoder's bits-read and PCM for that stream.  For every hand-assembled decoder case, the real decoder's.
Data only: digests of what the reference's compiled code produced, no source text."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fullref_cases import ENC_CASES, DEC_ONLY, enc_case, have_driver, driver_encode, driver_decode, payload, enc_digest, dec_digest  # noqa: E402


def main():
    assert have_driver(), "needs oracle/_ref/ulc_ref_driver (make -C oracle ref)"
    out = {"encode": {}, "decode_only": {}}
    for tag in ENC_CASES:
        pcm, bs, rate, mode, p0, p1 = enc_case(tag)
        r = driver_encode(pcm, bs, rate, mode, p0, p1)
        bits, dpcm = driver_decode(r["out"], pcm.shape[1], bs)
        out["encode"][tag] = {"blocks": int(len(r["bits"])), "bytes": int(sum(len(p) for p in payload(r))),
                              "stream_sha256": enc_digest(r), "decode_sha256": dec_digest(bits, dpcm)}
    for tag in DEC_ONLY:
        blocks, bs, ch = DEC_ONLY[tag]()
        bits, dpcm = driver_decode(blocks, ch, bs)
        out["decode_only"][tag] = {"blocks": int(len(bits)), "decode_sha256": dec_digest(bits, dpcm)}
    json.dump(out, open(os.path.join(HERE, "fullref_digests.json"), "w"), indent=1, sort_keys=True)
    print(len(out["encode"]), "encoder cases,", len(out["decode_only"]), "decoder-only cases")


if __name__ == "__main__":
    main()
