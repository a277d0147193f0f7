"""Wall clock of the sample-crop call (ulcx_decode_crops_samples_dev) beside what a loader does without it: synchronised calls
on device buffers, 20 timed calls per form after a warm-up, the forms alternating in one process (tools/crops_bench.py's pattern).

    python tools/sample_crops_bench.py [--steps N] [--warmup W] [--out FILE]

4096 rows of nSamples = 30 * 2048 + 1 samples of stereo 2048 at random sample starts of a corpus of 64 files of 40 blocks
(random file per row); a row touches up to nB = 31 blocks.  The forms:
  samples      the sample-crop call: [4096][2][nSamples], channels-first, trimmed and offset at the store
  crops        (a) ulcx_decode_crops_dev of nB blocks on the same rows (first = start / 2048), alone: [4096][31][2048][2]
  crops+torch  (b) that call followed by the torch glue a loader needs behind it: gather at the row's own offset, transpose,
               contiguous()
  crops+torch1 (b') the same glue written as ONE pass: a gather from the transposed view straight into the contiguous result
Before anything is timed the sample-crop output is compared bit for bit with (b)'s and (b')'s.
`samples_over_crops`: the distance from (a), medians; `samples_median_within_crops_spread`: the best case.  `samples_over_crops_torch`
(< 1: the claim) and its one-pass sibling.  One JSON line with the library's build revision, appended to --out (default
profiles/sample_crops_bench.txt)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_crops_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize

    bs, ch, rate, F, K, n = 2048, 2, 44100, 64, 40, 4096
    nS = 30 * bs + 1
    nB = ulc_amd.crop_blocks(bs, nS)
    assert nB == 31
    # the corpus of tools/crops_bench.py: 16 distinct synthetic streams tiled to 64 files, encoded at VBR 50 and packed as the tool writes them
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

    dec = ulc_amd.BatchDecoder(n, ch, bs, nB + 1)
    d_idx = torch.zeros((F, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    dec.index_packed_rows_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
    sync()
    assert int(d_cnt.min().item()) == K, "every file has 40 whole blocks"
    rng = np.random.default_rng(3)
    files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
    h_start = rng.integers(0, K * bs - nS + 1, n).astype(np.int64)
    start = torch.from_numpy(h_start).to(dev)
    first = torch.from_numpy((h_start // bs).astype(np.int32)).to(dev)
    skip = torch.from_numpy(h_start % bs).to(dev)
    take = skip[:, None] + torch.arange(nS, device=dev)[None, :]                    # [n][nS] sample of the row's blocks each output sample is
    o_samp = torch.zeros((n, ch, nS), dtype=torch.float32, device=dev)
    o_crop = torch.zeros((n, nB, bs, ch), dtype=torch.float32, device=dev)
    b_samp = torch.zeros((n, nB), dtype=torch.int32, device=dev)
    b_crop = torch.zeros((n, nB), dtype=torch.int32, device=dev)
    glued = {}
    stages = {k: ([], []) for k in ("samples", "crops")}

    def note(k):
        sync()
        st = dec.stage_ms()
        stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])

    def samples():
        dec.decode_crops_samples_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(),
                                     start.data_ptr(), 0, nS, o_samp.data_ptr(), b_samp.data_ptr())

    def crops():
        dec.decode_crops_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(),
                             first.data_ptr(), 0, nB, o_crop.data_ptr(), b_crop.data_ptr())

    def crops_torch():
        crops()
        rows = o_crop.view(n, nB * bs, ch)
        glued["three"] = torch.gather(rows, 1, take[:, :, None].expand(-1, -1, ch)).transpose(1, 2).contiguous()

    def crops_torch1():
        crops()
        rows = o_crop.view(n, nB * bs, ch).transpose(1, 2)
        glued["one"] = torch.gather(rows, 2, take[:, None, :].expand(-1, ch, -1))

    samples(); crops_torch(); crops_torch1(); sync()
    same = bool(torch.equal(o_samp.view(torch.int32), glued["three"].view(torch.int32)) and torch.equal(o_samp.view(torch.int32), glued["one"].view(torch.int32))
                and glued["three"].is_contiguous() and glued["one"].is_contiguous())
    # (the sizes: the sample call reports 0 for a 31st block the row does not touch, the block call decodes it)
    touched = torch.arange(nB, device=dev)[None, :] <= ((skip + nS - 1) // bs)[:, None]
    same_bits = bool(torch.equal(b_samp, torch.where(touched, b_crop, torch.zeros_like(b_crop))))
    r = timed({"samples": samples, "crops": crops, "crops+torch": crops_torch, "crops+torch1": crops_torch1}, a.steps, a.warmup, sync)
    for _ in range(a.steps):                                # the stages' device time, outside the wall-clock loop (reading it waits for the device)
        samples(); note("samples")
        crops(); note("crops")
    samples(); sync(); cut_samples = list(dec.last_cut())
    crops(); sync(); cut_crops = list(dec.last_cut())
    s = {k: stats(v) for k, v in r.items()}
    ratio = lambda x, y: round(s[x]["median_ms"] / s[y]["median_ms"], 4)
    line = {"what": "4096 rows x (30 * 2048 + 1) samples of stereo 2048 at random sample starts of a 64-file corpus: the sample-crop call beside "
                    "(a) the block crop call of 31 blocks alone, (b) that call + torch gather / transpose / contiguous, (b') + a one-pass gather "
                    "(wall clock; scan / syn: device time of the stages, the sample call's scan with its row prologue)",
            "samples": s["samples"], "crops": s["crops"], "crops_torch": s["crops+torch"], "crops_torch_one_pass": s["crops+torch1"],
            "samples_over_crops": ratio("samples", "crops"),
            "samples_median_within_crops_spread": bool(s["crops"]["min_ms"] <= s["samples"]["median_ms"] <= s["crops"]["max_ms"]),
            "samples_over_crops_torch": ratio("samples", "crops+torch"), "samples_over_crops_torch_one_pass": ratio("samples", "crops+torch1"),
            "samples_scan": stats(stages["samples"][0]), "samples_syn": stats(stages["samples"][1]),
            "crops_scan": stats(stages["crops"][0]), "crops_syn": stats(stages["crops"][1]),
            "outputs_equal": same, "bits_equal_on_touched_blocks": same_bits, "rows_touching_31_blocks": int(touched[:, nB - 1].sum().item()),
            "cut_of_sample_call": cut_samples, "cut_of_crop_call": cut_crops,
            "output_bytes_samples": nbytes(o_samp), "output_bytes_crops": nbytes(o_crop), "ulcx_build_rev": rev}
    dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
