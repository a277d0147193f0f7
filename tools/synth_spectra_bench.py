"""Wall clock of the synth call (ulcx_synth_spectra_dev) beside the sample-crop call that yields the same PCM and beside a plain
copy of the bytes it moves: synchronised calls on device buffers, 20 timed calls per form after a warm-up, the forms alternating
in one process (tools/crops_bench.py's pattern).

    python tools/synth_spectra_bench.py [--steps N] [--warmup W] [--out FILE]

4096 rows x 31 output blocks of stereo 2048 on tools/spectra_bench.py's corpus (64 files of 40 blocks, random file, random start
>= 1).  The planes come from ulcx_decode_crops_spectra_dev(first - 1, 32 blocks): plane 0 is the block in front (ULCX_SYNTH_WARM).
The forms:
  synth       ulcx_synth_spectra_dev, flags WARM: the coded mid / side planes -> [n][2][31 * 2048] samples
  synth_lr    flags WARM | ULCX_SPECTRA_LR on the planes of the LR spectra call (no un-mix)
  samples     ulcx_decode_crops_samples_dev of 31 * 2048 samples from sample first * 2048 of the same files: the same PCM, from the bytes
  copy        a device-to-device copy of the output's size out of the planes: the bytes the synth call must at least move
Before anything is timed: synth == samples bit for bit (the WARM identity, include/ulc_amd.h), and the largest difference of the LR
route.  prologue / syn: device time of the call's two stages (ulcx_decoder_stage_ms: k_synth_rows or the crop walk; the synthesis
kernel), taken outside the wall-clock loop.  One JSON line with the library's build revision, appended to --out (default
profiles/synth_spectra_bench.txt).  Not measured: other geometries, PCM16, the host form, corpus.synth_spectra."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from crops_bench import timed, stats, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_spectra_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize
    WARM, LR = ulc_amd.SYNTH_WARM, ulc_amd.SPECTRA_LR

    bs, ch, rate, F, K, N, n = 2048, 2, 44100, 64, 40, 31, a.rows
    # the corpus of tools/spectra_bench.py: 16 distinct synthetic streams tiled to 64 files, encoded at VBR 50 and packed as the tool writes them
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(F) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(F, ch, bs, rate, K)
    d_slots = torch.zeros((F, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((F, K), dtype=torch.int32, device=dev)
    enc.encode_dev(d_pcm.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    sync()
    stride = (int(((d_bits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    pay = torch.zeros((F, stride), dtype=torch.uint8, device=dev)
    nb = torch.zeros(F, dtype=torch.int32, device=dev)
    assert ulc_amd.lib().ulcx_pack_streams_dev(0, F, K, enc.slot, d_slots.data_ptr(), d_bits.data_ptr(), pay.data_ptr(), stride, nb.data_ptr(), None, None) == 0
    sync()
    enc.close()
    del d_slots, d_pcm

    dec = ulc_amd.BatchDecoder(n, ch, bs, N + 2)
    d_idx = torch.zeros((F, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    dec.index_packed_rows_dev(F, pay.data_ptr(), stride, nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
    sync()
    assert int(d_cnt.min().item()) == K, "every file has its whole blocks"
    rng = np.random.default_rng(3)
    files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
    first_np = rng.integers(1, K - N + 1, n).astype(np.int32)
    front = torch.from_numpy(first_np - 1).to(dev)
    start = torch.from_numpy(first_np.astype(np.int64) * bs).to(dev)
    # the planes, once: the spectra call from the block in front, N + 1 blocks per row
    coef = {k: torch.zeros((n, ch, N + 1, bs), dtype=torch.float32, device=dev) for k in ("synth", "synth_lr")}
    wc = torch.zeros((n, N + 1), dtype=torch.int32, device=dev)
    sbits = torch.zeros((n, N + 1), dtype=torch.int32, device=dev)
    for k, fl in (("synth", 0), ("synth_lr", LR)):
        dec.decode_crops_spectra_dev(F, pay.data_ptr(), stride, nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(), front.data_ptr(), 0,
                                     N + 1, fl, coef[k].data_ptr(), wc.data_ptr(), sbits.data_ptr())
    sync()
    assert int((sbits > 0).sum().item()) == n * (N + 1)
    out = {k: torch.zeros((n, ch, N * bs), dtype=torch.float32, device=dev) for k in ("synth", "synth_lr", "samples", "copy")}
    live = torch.zeros((n, N), dtype=torch.int32, device=dev)
    cbits = torch.zeros((n, ulc_amd.crop_blocks(bs, N * bs)), dtype=torch.int32, device=dev)

    def synth(label, flags):
        return lambda: dec.synth_spectra_dev(n, N + 1, flags, coef[label].data_ptr(), wc.data_ptr(), out[label].data_ptr(), live.data_ptr())

    def samples():
        dec.decode_crops_samples_dev(F, pay.data_ptr(), stride, nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(), start.data_ptr(), 0,
                                     N * bs, out["samples"].data_ptr(), cbits.data_ptr())

    src = coef["synth"].view(-1)[:out["copy"].numel()]

    def copy():
        out["copy"].view(-1).copy_(src)

    fns = {"synth": synth("synth", WARM), "synth_lr": synth("synth_lr", WARM | LR), "samples": samples, "copy": copy}
    for fn in fns.values():
        fn()
    sync()
    identity = bool(torch.equal(out["synth"].view(torch.int32), out["samples"].view(torch.int32)) and int(live.sum().item()) == n * N)
    lr_diff = float((out["synth_lr"] - out["samples"]).abs().max().item())
    peak = float(out["samples"].abs().max().item())
    r = timed(fns, a.steps, a.warmup, sync)
    stages = {k: ([], []) for k in ("synth", "synth_lr", "samples")}
    for _ in range(a.steps):                                # the stages' device time, outside the wall-clock loop (reading it waits for the device)
        for k in stages:
            fns[k](); sync()
            st = dec.stage_ms()
            stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])
    fns["synth"](); sync(); cut_synth = list(dec.last_cut())
    samples(); sync(); cut_samples = list(dec.last_cut())
    s = {k: stats(v) for k, v in r.items()}
    moved = nbytes(coef["synth"]) + nbytes(out["synth"])
    line = {"what": f"{n} rows x {N} output blocks of stereo {bs}: the synth call (WARM; flags 0 and LR) beside the sample-crop call that yields the same PCM and "
                    "a device copy of the output's size (wall clock; prologue / walk / syn: device time of the stages)",
            "synth": s["synth"], "synth_lr": s["synth_lr"], "samples": s["samples"], "copy": s["copy"],
            "synth_over_samples": round(s["synth"]["median_ms"] / s["samples"]["median_ms"], 4),
            "synth_over_copy": round(s["synth"]["median_ms"] / s["copy"]["median_ms"], 4),
            "lr_over_synth": round(s["synth_lr"]["median_ms"] / s["synth"]["median_ms"], 4),
            "synth_prologue": stats(stages["synth"][0]), "synth_syn": stats(stages["synth"][1]),
            "synth_lr_prologue": stats(stages["synth_lr"][0]), "synth_lr_syn": stats(stages["synth_lr"][1]),
            "samples_walk": stats(stages["samples"][0]), "samples_syn": stats(stages["samples"][1]),
            "synth_syn_over_samples_syn": round(stats(stages["synth"][1])["median_ms"] / stats(stages["samples"][1])["median_ms"], 4),
            "synth_equals_samples_bit_for_bit": identity, "lr_route_max_abs_diff": lr_diff, "pcm_peak": peak,
            "bytes_in_planes": nbytes(coef["synth"]), "bytes_out_pcm": nbytes(out["synth"]), "bytes_copy_moves": 2 * nbytes(out["copy"]),
            "synth_GB_per_s_moved": round(moved / (s["synth"]["median_ms"] * 1e-3) / 1e9, 1),
            "synth_syn_GB_per_s_moved": round(moved / (stats(stages["synth"][1])["median_ms"] * 1e-3) / 1e9, 1),
            "copy_GB_per_s_moved": round(2 * nbytes(out["copy"]) / (s["copy"]["median_ms"] * 1e-3) / 1e9, 1),
            "cut_of_synth_call": cut_synth, "cut_of_samples_call": cut_samples, "ulcx_build_rev": rev}
    dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
