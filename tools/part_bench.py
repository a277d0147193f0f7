"""Wall clock of the mid crop call (ulcx_decode_crops_part_dev, ULCX_PART_MID) at lgD 0 .. 3 beside what a mono loader does without
it: the stereo sample-crop / low-rate call on the same rows, alone and followed by the cheapest torch fold, torch.mean(dim=1).
Synchronised calls on device buffers, 20 timed calls per form after a warm-up, the forms alternating in one process
(tools/lowrate_bench.py's pattern and corpus).

    python tools/part_bench.py [--steps N] [--warmup W] [--out FILE] [--stereo-only]

4096 rows at random block-unaligned starts of a corpus of 64 stereo 2048 files of 40 blocks (random file per row).  Every row covers
the time span of 30 full blocks: 61440 / D samples from reduced sample t0, D = 1 << lgD.  The forms:
  stereo/D       ulcx_decode_crops_samples_dev (D = 1) / ulcx_decode_crops_lowrate_dev, [4096][2][61440 / D]: the baseline, unchanged
  stereo+mean/D  that call, then torch.mean(dim=1) over its output
  mid/D          ulcx_decode_crops_part_dev with ULCX_PART_MID, [4096][1][61440 / D]
  side/1         the same with ULCX_PART_SIDE at full rate
  long:...       stereo/1 and mid/1 over 64 rows of the same span (31 blocks touched): the part call launches one workgroup per row
                 and has no cut, the stereo call cuts its rows evenly over the device
`X_minus_Y`: the difference of the medians beside the sum of the two spreads (max - min); `gain` is true only where the difference
exceeds that sum.  scan / syn: device time of the two stages (the scan with its row prologue).  --stereo-only: the stereo forms
alone - what a build without the part entries (the parent's, named by ULC_AMD_LIB) can run, for the headline row.  One JSON line
with the library's build revision, appended to --out (default profiles/part_bench.txt)."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crops_bench import timed, stats, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_bench.txt"))
    ap.add_argument("--stereo-only", action="store_true")
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize

    bs, ch, rate, F, K, n, n_long = 2048, 2, 44100, 64, 40, 4096, 64
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
    Ds = (1, 2, 4, 8)
    start = {D: torch.from_numpy(h_start // D).to(dev) for D in Ds}
    o_st = {D: torch.zeros((n, ch, span // D), dtype=torch.float32, device=dev) for D in Ds}
    o_mid = {D: torch.zeros((n, 1, span // D), dtype=torch.float32, device=dev) for D in Ds}
    bits = torch.zeros((n, nB), dtype=torch.int32, device=dev)
    corpus = (F, d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr())
    kept = {}

    def stereo(D, rows=n):
        lg = D.bit_length() - 1
        def run():
            if D == 1:
                dec.decode_crops_samples_dev(*corpus, rows, files.data_ptr(), start[1].data_ptr(), 0, span, o_st[1].data_ptr(), bits.data_ptr())
            else:
                dec.decode_crops_lowrate_dev(*corpus, rows, files.data_ptr(), start[D].data_ptr(), 0, span // D, lg, o_st[D].data_ptr(), bits.data_ptr())
        return run

    def stereo_mean(D):
        call = stereo(D)
        def run():
            call()
            kept[D] = torch.mean(o_st[D], dim=1)
        return run

    def part(D, which, rows=n):
        lg = D.bit_length() - 1
        def run():
            dec.decode_crops_part_dev(*corpus, rows, files.data_ptr(), start[D].data_ptr(), 0, span // D, lg, which, o_mid[D].data_ptr(), bits.data_ptr())
        return run

    forms = {}
    for D in Ds:
        forms[f"stereo/{D}"] = stereo(D)
        forms[f"stereo+mean/{D}"] = stereo_mean(D)
        if not a.stereo_only:
            forms[f"mid/{D}"] = part(D, ulc_amd.PART_MID)
    if not a.stereo_only:
        forms["side/1"] = part(1, ulc_amd.PART_SIDE)
        forms["long:mid/1"] = part(1, ulc_amd.PART_MID, n_long)
    forms["long:stereo/1"] = stereo(1, n_long)
    for fn in forms.values():
        fn()
    sync()
    line = {"what": "4096 rows x the span of 30 blocks of stereo 2048 from a 64-file corpus: the mid crop call at lgD 0 .. 3 beside the stereo sample-crop / "
                    "low-rate call on the same rows, alone and followed by torch.mean(dim=1); long: 64 rows of the same span (wall clock; scan / syn: "
                    "device time of the stages)"}
    if not a.stereo_only:
        # what mono means: the coded mid against the fold of the stereo decode, in units of the fold's two roundings
        part(1, ulc_amd.PART_MID)(); stereo(1)(); sync()
        fold = o_st[1].double().mean(dim=1)
        err = (o_mid[1][:, 0].double() - fold).abs()
        line["mid_vs_fold"] = {"largest_abs_difference": float(err.max().item()), "samples_that_differ": int((err > 0).sum().item()), "samples": int(err.numel()),
                               "largest_sample": float(fold.abs().max().item())}
        line["mid_outputs_finite_and_nonzero"] = {D: bool(torch.isfinite(o_mid[D]).all().item() and (o_mid[D] != 0).any(dim=2).all().item()) for D in Ds}
        del fold, err
    r = timed(forms, a.steps, a.warmup, sync)
    staged = [k for k in forms if "+" not in k]
    stages = {k: ([], []) for k in staged}
    cuts = {}
    for _ in range(a.steps):                                # the stages' device time, outside the wall-clock loop (reading it waits for the device)
        for k in staged:
            forms[k](); sync()
            st = dec.stage_ms()
            stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])
            cuts[k] = list(dec.last_cut())
    s = {k: stats(v) for k, v in r.items()}
    spread = lambda k: s[k]["max_ms"] - s[k]["min_ms"]
    line.update(s)

    def versus(x, y, of=s, sp=spread):
        diff, both = of[y]["median_ms"] - of[x]["median_ms"], sp(x) + sp(y)
        return {"median_difference_ms": round(diff, 4), "sum_of_spreads_ms": round(both, 4), "ratio": round(of[x]["median_ms"] / of[y]["median_ms"], 4), "gain": bool(diff > both)}
    if not a.stereo_only:
        for D in Ds:
            line[f"mid/{D}_minus_stereo/{D}"] = versus(f"mid/{D}", f"stereo/{D}")
            line[f"mid/{D}_minus_stereo+mean/{D}"] = versus(f"mid/{D}", f"stereo+mean/{D}")
        line["long:mid/1_minus_long:stereo/1"] = versus("long:mid/1", "long:stereo/1")
    syn = {k: stats(stages[k][1]) for k in staged}
    for k in staged:
        line[k + "_scan"] = stats(stages[k][0]); line[k + "_syn"] = syn[k]; line[k + "_cut"] = cuts[k]
    if not a.stereo_only:
        sps = lambda k: syn[k]["max_ms"] - syn[k]["min_ms"]
        for D in Ds:
            line[f"syn:mid/{D}_minus_stereo/{D}"] = versus(f"mid/{D}", f"stereo/{D}", syn, sps)
    line.update({"output_bytes_stereo": {D: nbytes(o_st[D]) for D in Ds}, "output_bytes_mid": {D: nbytes(o_mid[D]) for D in Ds}, "ulcx_build_rev": rev})
    dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
