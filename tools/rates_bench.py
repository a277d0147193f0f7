"""Wall clock of ulcx_encode_dev_rates against the scalar ulcx_encode_dev (synchronised calls, device buffers).

    python tools/rates_bench.py [--steps N] [--warmup W]

Shapes: a uniform VBR 50 table at the headline shape (4096 stereo streams x 32 blocks of 2048), a uniform CBR 64 table at
4096 x 16 at 48 kHz, and a 50/50 VBR 50 / CBR 64 mix at 4096 x 16 (against the scalar CBR call).  Prints one JSON line
per shape with the median ms of each form and their ratio."""
import argparse
import json
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ulc_amd  # noqa: E402
from ulc_testlib import synth_pcm  # noqa: E402


def run(name, B, K, rate, table, mode, p0, steps, warmup):
    bs, ch = 2048, 2
    dev = torch.device("cuda:0")
    # a few distinct synthetic streams tiled over the batch (the content only has to be realistic, not unique)
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    enc.set_timing(False)
    d_out = torch.empty((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.empty((B, K), dtype=torch.int32, device=dev)
    d_rate = torch.tensor(table, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)

    def scalar():
        enc.encode_dev(d_pcm.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), mode=mode, p0=p0, stream=st.cuda_stream)

    def rates():
        enc.encode_dev_rates(d_rate.data_ptr(), d_pcm.data_ptr(), K, d_out.data_ptr(), d_bits.data_ptr(), stream=st.cuda_stream)

    res = {}
    for label, fn in (("scalar", scalar), ("rates", rates), ("scalar2", scalar), ("rates2", rates)):
        for _ in range(warmup):
            fn()
        st.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            st.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[label] = ts
    enc.close()
    sc = float(np.median(res["scalar"] + res["scalar2"]))
    rt = float(np.median(res["rates"] + res["rates2"]))
    print(json.dumps({"shape": name, "streams": B, "blocks": K, "rate_hz": rate, "scalar_ms": round(sc, 3), "rates_ms": round(rt, 3),
                      "ratio": round(rt / sc, 4), "steps": 2 * steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B = 4096
    run("vbr50_uniform", B, 32, 44100, [(-50.0, 0.0)] * B, ulc_amd.MODE_VBR, 50.0, a.steps, a.warmup)
    run("cbr64_48k_uniform", B, 16, 48000, [(64.0, 0.0)] * B, ulc_amd.MODE_CBR, 64.0, a.steps, a.warmup)
    run("vbr50_cbr64_mix", B, 16, 48000, [(-50.0, 0.0) if s % 2 == 0 else (64.0, 0.0) for s in range(B)], ulc_amd.MODE_CBR, 64.0,
        a.steps, a.warmup)


if __name__ == "__main__":
    main()
