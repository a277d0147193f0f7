"""Wall clock of the low-rate sample-crop call (ulcx_decode_crops_lowrate_dev) at D = 2, 4, 8 beside what a loader does without
it: the full-rate sample-crop call on the same time spans, alone and followed by a strided torch FIR decimation.  Synchronised calls
on device buffers, 20 timed calls per form after a warm-up, the forms alternating in one process (tools/crops_bench.py's pattern).

    python tools/lowrate_bench.py [--steps N] [--warmup W] [--out FILE]

4096 rows at random block-unaligned starts of a corpus of 64 stereo 2048 files of 40 blocks (random file per row; the corpus of
tools/sample_crops_bench.py).  Every row covers the time span of 30 full blocks: 61440 samples at full rate from sample D * t0,
61440 / D reduced samples from reduced sample t0.  The forms:
  full         ulcx_decode_crops_samples_dev, [4096][2][61440]: the unchanged full-rate path, the baseline
  full+fir/D   that call, then torch.nn.functional.conv1d with stride D over its output (a windowed-sinc low-pass of 16 D + 1 taps)
  low/D        ulcx_decode_crops_lowrate_dev at lgD = log2 D, [4096][2][61440 / D]
`faster_by_more_than_the_spreads` (per D): full's median minus low's exceeds (max - min) of both together - the claim for D = 2.
scan / syn: device time of the two stages (the scan with its row prologue).  One JSON line with the library's build revision,
appended to --out (default profiles/lowrate_bench.txt)."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crops_bench import timed, stats, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowrate_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize

    bs, ch, rate, F, K, n = 2048, 2, 44100, 64, 40, 4096
    span = 30 * bs
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_in = torch.from_numpy(np.ascontiguousarray(base[np.arange(F) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(F, ch, bs, rate, K)
    d_slots = torch.zeros((F, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((F, K), dtype=torch.int32, device=dev)
    enc.encode_dev(d_in.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    sync()
    stride = (int(((d_bits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    d_pay = torch.zeros((F, stride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(F, dtype=torch.int32, device=dev)
    assert ulc_amd.lib().ulcx_pack_streams_dev(0, F, K, enc.slot, d_slots.data_ptr(), d_bits.data_ptr(), d_pay.data_ptr(), stride,
                                               d_nb.data_ptr(), None, None) == 0
    sync()
    enc.close()
    del d_slots, d_in

    nB = ulc_amd.crop_blocks(bs, span)
    dec = ulc_amd.BatchDecoder(n, ch, bs, nB + 1)
    d_idx = torch.zeros((F, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    dec.index_packed_rows_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
    sync()
    assert int(d_cnt.min().item()) == K, "every file has 40 whole blocks"
    rng = np.random.default_rng(3)
    files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
    h_start = (rng.integers(0, (K * bs - span) // 8 + 1, n) * 8).astype(np.int64)      # full-rate starts: multiples of 8, so every ratio starts on its own sample
    start = {D: torch.from_numpy(h_start // D).to(dev) for D in (1, 2, 4, 8)}
    o_full = torch.zeros((n, ch, span), dtype=torch.float32, device=dev)
    o_low = {D: torch.zeros((n, ch, span // D), dtype=torch.float32, device=dev) for D in (2, 4, 8)}
    bits = torch.zeros((n, nB), dtype=torch.int32, device=dev)
    corpus = (F, d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr())

    def fir(D):
        taps = 16 * D + 1
        t = torch.arange(taps, dtype=torch.float64) - (taps - 1) / 2
        h = torch.sinc(t / D) / D * torch.hann_window(taps, periodic=False, dtype=torch.float64)
        return (h / h.sum()).to(torch.float32).to(dev).view(1, 1, taps)
    firs = {D: fir(D) for D in (2, 4, 8)}
    kept = {}

    def full():
        dec.decode_crops_samples_dev(*corpus, n, files.data_ptr(), start[1].data_ptr(), 0, span, o_full.data_ptr(), bits.data_ptr())

    def full_fir(D):
        def run():
            full()
            kept[D] = torch.nn.functional.conv1d(o_full.view(n * ch, 1, span), firs[D], stride=D, padding=8 * D).view(n, ch, -1)
        return run

    def low(D):
        lg = D.bit_length() - 1
        def run():
            dec.decode_crops_lowrate_dev(*corpus, n, files.data_ptr(), start[D].data_ptr(), 0, span // D, lg, o_low[D].data_ptr(), bits.data_ptr())
        return run

    forms = {"full": full}
    for D in (2, 4, 8):
        forms[f"full+fir/{D}"] = full_fir(D)
        forms[f"low/{D}"] = low(D)
    for fn in forms.values():
        fn()
    sync()
    sane = {D: bool(torch.isfinite(o_low[D]).all().item() and (o_low[D] != 0).any(dim=2).all().item()) for D in (2, 4, 8)}
    r = timed(forms, a.steps, a.warmup, sync)
    stages = {k: ([], []) for k in ("full", "low/2", "low/4", "low/8")}
    cuts = {}
    for _ in range(a.steps):                                # the stages' device time, outside the wall-clock loop (reading it waits for the device)
        for k in stages:
            forms[k](); sync()
            st = dec.stage_ms()
            stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])
            cuts[k] = list(dec.last_cut())
    s = {k: stats(v) for k, v in r.items()}
    spread = lambda k: s[k]["max_ms"] - s[k]["min_ms"]
    line = {"what": "4096 rows x the span of 30 blocks of stereo 2048 from a 64-file corpus: the low-rate sample-crop call at D = 2, 4, 8 beside the "
                    "full-rate sample-crop call on the same spans, alone and followed by a strided torch FIR decimation (wall clock; scan / syn: "
                    "device time of the stages)"}
    line.update({k: v for k, v in s.items()})
    for D in (2, 4, 8):
        line[f"low/{D}_over_full"] = round(s[f"low/{D}"]["median_ms"] / s["full"]["median_ms"], 4)
        line[f"low/{D}_over_full+fir"] = round(s[f"low/{D}"]["median_ms"] / s[f"full+fir/{D}"]["median_ms"], 4)
        line[f"low/{D}_faster_by_more_than_the_spreads"] = bool(s["full"]["median_ms"] - s[f"low/{D}"]["median_ms"] > spread("full") + spread(f"low/{D}"))
    for k in stages:
        line[k + "_scan"] = stats(stages[k][0]); line[k + "_syn"] = stats(stages[k][1]); line[k + "_cut"] = cuts[k]
    line.update({"low_outputs_finite_and_nonzero": sane, "output_bytes_full": nbytes(o_full), "output_bytes_low": {D: nbytes(o_low[D]) for D in (2, 4, 8)},
                 "ulcx_build_rev": rev})
    dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
