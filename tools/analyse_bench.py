"""Wall clock of the analysis-only call (ulcx_analyse_dev) against the VBR 50 encode call (ulcx_encode_dev) on the same
encoder and input: synchronised calls, device buffers, the two forms alternating in one process.

    python tools/analyse_bench.py [--steps N] [--warmup W] [--variant xfa|kxf]

Shapes: the headline shape (4096 stereo streams x 32 blocks of 2048 at 44.1 kHz) with float and with PCM16 input, and the
window-switching configuration's (2048 streams x 16 blocks of 4096 at 48 kHz).  One JSON line per shape with the median ms
of each form and their ratio.  --variant kxf times the plain launch subset instead (the analysis call on the encode call's
transform kernel, ULCX_ANALYSE_KXF=1: a timing comparison, not a configuration to ship)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(name, variant, B, K, bs, rate, pcm16, steps, warmup):
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    ch = 2
    dev = torch.device("cuda:0")
    # a few distinct synthetic streams tiled over the batch (the content only has to be realistic, not unique)
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    if pcm16:
        base = np.clip(np.rint(base * 32768.0), -32768, 32767).astype(np.int16)
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    enc.set_timing(False)
    d_out = torch.empty((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.empty((B, K), dtype=torch.int32, device=dev)
    d_wc = torch.empty((B, K), dtype=torch.int32, device=dev)
    d_cplx = torch.empty((B, K), dtype=torch.float32, device=dev)
    e_wc, e_cplx = torch.empty_like(d_wc), torch.empty_like(d_cplx)
    st = torch.cuda.current_stream(dev)

    def encode():
        fn = enc.encode_dev_pcm16 if pcm16 else enc.encode_dev
        fn(d_pcm.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), e_wc.data_ptr(), e_cplx.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0,
           stream=st.cuda_stream)

    def analyse():
        enc.analyse_dev(d_pcm.data_ptr(), K, d_wc.data_ptr(), d_cplx.data_ptr(), stream=st.cuda_stream, pcm16=pcm16)

    res = {"encode": [], "analyse": []}
    for rep in range(2):
        for label, fn in (("encode", encode), ("analyse", analyse)):
            enc.reset()                                            # (both forms time the same blocks of the same streams)
            for _ in range(warmup):
                fn()
            st.synchronize()
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()
                st.synchronize()
                res[label].append((time.perf_counter() - t0) * 1e3)
    # both forms leave the same values behind (same calls since the reset)
    same = bool(torch.equal(d_wc, e_wc) and torch.equal(d_cplx.view(torch.int32), e_cplx.view(torch.int32)))
    enc.close()
    em, am = float(np.median(res["encode"])), float(np.median(res["analyse"]))
    print(json.dumps({"shape": name, "variant": variant, "streams": B, "blocks": K, "block_size": bs, "rate_hz": rate,
                      "input": "pcm16" if pcm16 else "float", "encode_ms": round(em, 3), "analyse_ms": round(am, 3),
                      "ratio": round(am / em, 4), "encode_min_max": [round(min(res["encode"]), 3), round(max(res["encode"]), 3)],
                      "analyse_min_max": [round(min(res["analyse"]), 3), round(max(res["analyse"]), 3)],
                      "steps": 2 * steps, "outputs_equal": same, "build": ulc_amd.build_rev()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per form and round (two rounds, forms alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", choices=("xfa", "kxf"), default="xfa")
    ap.add_argument("--shapes", default="headline,headline_pcm16,wswitch_4096")
    a = ap.parse_args()
    if a.variant == "kxf":
        os.environ["ULCX_ANALYSE_KXF"] = "1"                       # read when an encoder is created
    else:
        os.environ.pop("ULCX_ANALYSE_KXF", None)
    shapes = {"headline": (4096, 32, 2048, 44100, False), "headline_pcm16": (4096, 32, 2048, 44100, True),
              "wswitch_4096": (2048, 16, 4096, 48000, False)}
    for name in a.shapes.split(","):
        run(name, a.variant, *shapes[name], a.steps, a.warmup)


if __name__ == "__main__":
    main()
