"""Wall clock of the distortion call (ulcx_decode_crops_distortion_dev) beside what it replaces: synchronised calls on device
buffers, 20 timed calls per form after a warm-up, the forms alternating in one process (tools/spectra_bench.py's pattern).

    python tools/distortion_bench.py [--steps N] [--warmup W] [--out FILE]

The shape: 4096 rows x 31 blocks of stereo 2048 drawn from a corpus of 64 files of 40 blocks (random file, random start), nSeg 16;
the reference is [4096][2][31][2048] float32 planes, row i for crop row i.  The forms:
  (a) dist         the call with the reference
  (b) dist_noref   the call with d_ref = NULL
  (c) spectra_torch  today's path: ulcx_decode_crops_spectra_dev into planes, then a torch float64 reduction of both planes to the
                   same [n][2][31][16][3] shape
  (d) spectra      the spectra call alone
  (e) copy         a device copy of the bytes form (a) reads: the reference planes
dist_kernel / spectra_expand: device time of the calls' second stage (ulcx_decoder_stage_ms), taken outside the wall-clock loop.
Before anything is timed the call's output is compared bit for bit with the numpy referee (tests/distortion_testlib.py) on a
subsample of the rows, the referee fed with the spectra call's planes.  No ratio is fixed in advance: `a_gains_over_c` is true only
when the medians differ by more than the two spreads together.  One JSON line with the library's build revision, appended to --out
(default profiles/distortion_bench.txt)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    import distortion_testlib as T
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize

    bs, ch, rate, F, K, N, n, n_seg = 2048, 2, 44100, 64, 40, 31, 4096, 16
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

    dec = ulc_amd.BatchDecoder(n, ch, bs, N + 1)
    d_idx = torch.zeros((F, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    dec.index_packed_rows_dev(F, pay.data_ptr(), stride, nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
    sync()
    assert int(d_cnt.min().item()) == K, "every file has its whole blocks"
    rng = np.random.default_rng(3)
    files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
    first = torch.from_numpy(rng.integers(0, K - N + 1, n).astype(np.int32)).to(dev)
    coef = torch.zeros((n, ch, N, bs), dtype=torch.float32, device=dev)
    wc = torch.zeros((n, N), dtype=torch.int32, device=dev)
    bits = torch.zeros((n, N), dtype=torch.int32, device=dev)
    dist = {k: torch.zeros((n, ch, N, n_seg, 3), dtype=torch.float64, device=dev) for k in ("dist", "dist_noref", "spectra_torch")}

    def spectra():
        dec.decode_crops_spectra_dev(F, pay.data_ptr(), stride, nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(), first.data_ptr(),
                                     0, N, 0, coef.data_ptr(), wc.data_ptr(), bits.data_ptr())

    # the reference: the coded planes themselves, perturbed - a clean spectrum's magnitudes, and an error that is not zero
    spectra(); sync()
    ref = (coef * 1.03125 + 0.001 * torch.randn(coef.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).contiguous()
    ref_copy = torch.empty_like(ref)

    def distortion(label, with_ref):
        return lambda: dec.decode_crops_distortion_dev(F, pay.data_ptr(), stride, nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(),
                                                       first.data_ptr(), 0, N, ref.data_ptr() if with_ref else 0, n if with_ref else 0, N if with_ref else 0, 0, 0,
                                                       n_seg, 0, dist[label].data_ptr(), wc.data_ptr(), bits.data_ptr())

    def spectra_torch():
        spectra()
        r, y = ref.view(n, ch, N, n_seg, bs // n_seg).double(), coef.view(n, ch, N, n_seg, bs // n_seg).double()
        o = dist["spectra_torch"]
        o[..., 0] = (r * r).sum(dim=-1); o[..., 1] = (y * y).sum(dim=-1); o[..., 2] = ((r - y) ** 2).sum(dim=-1)

    fns = {"dist": distortion("dist", True), "dist_noref": distortion("dist_noref", False), "spectra_torch": spectra_torch, "spectra": spectra,
           "copy": lambda: ref_copy.copy_(ref)}
    for fn in fns.values():
        fn()
    sync()
    # the referee on a subsample of the rows, before anything is timed
    rows = np.arange(0, n, 97)
    y_np, r_np = coef[rows].cpu().numpy(), ref[rows].cpu().numpy()
    exact = bool(T.same_bits64(dist["dist"][rows].cpu().numpy(), T.sums(r_np, y_np, n_seg))
                 and T.same_bits64(dist["dist_noref"][rows].cpu().numpy(), T.sums(np.zeros_like(y_np), y_np, n_seg)))
    assert exact, "the call's sums differ from the referee's"
    torch_rel = float(((dist["spectra_torch"] - dist["dist"]).abs() / dist["dist"].abs().clamp(min=1e-300)).max().item())

    r = timed(fns, a.steps, a.warmup, sync)
    stages = {k: [] for k in ("dist", "dist_noref", "spectra")}
    for _ in range(a.steps):                                # the second stage's device time, outside the wall-clock loop
        for k in stages:
            fns[k](); sync()
            stages[k].append(dec.stage_ms()["k_dsyn"])
    s = {k: stats(v) for k, v in r.items()}
    gap = s["spectra_torch"]["median_ms"] - s["dist"]["median_ms"]
    spreads = (s["dist"]["max_ms"] - s["dist"]["min_ms"]) + (s["spectra_torch"]["max_ms"] - s["spectra_torch"]["min_ms"])
    kern, rb = stats(stages["dist"]), nbytes(ref)
    line = {"what": "4096 rows x 31 blocks of stereo 2048 from a 64-file corpus, nSeg 16: the distortion call (a) with a reference, (b) without; (c) the "
                    "spectra call and a torch float64 reduction of both planes; (d) the spectra call alone; (e) a device copy of the reference (wall clock; "
                    "dist_kernel / spectra_expand: device time of the second stage)",
            "a_dist": s["dist"], "b_dist_noref": s["dist_noref"], "c_spectra_torch": s["spectra_torch"], "d_spectra": s["spectra"], "e_copy": s["copy"],
            "a_over_c": round(s["dist"]["median_ms"] / s["spectra_torch"]["median_ms"], 4), "a_over_d": round(s["dist"]["median_ms"] / s["spectra"]["median_ms"], 4),
            "a_gains_over_c": bool(gap > spreads), "c_minus_a_ms": round(gap, 4), "spreads_together_ms": round(spreads, 4),
            "dist_kernel": kern, "dist_noref_kernel": stats(stages["dist_noref"]), "spectra_expand": stats(stages["spectra"]),
            "dist_kernel_over_copy": round(kern["median_ms"] / s["copy"]["median_ms"], 4),
            "reference_bytes": rb, "plane_bytes_not_written": nbytes(coef), "dist_bytes": nbytes(dist["dist"]),
            "dist_kernel_reference_GB_per_s": round(rb / (kern["median_ms"] * 1e-3) / 1e9, 1),
            "bit_exact_against_the_referee_on_rows": int(rows.size), "torch_float64_max_relative_difference": torch_rel,
            "not_measured": ["other geometries and nSeg", "ULCX_SPECTRA_LR", "the host forms", "corpus.py's path", "hardware counters of k_ddist"],
            "ulcx_build_rev": rev}
    dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
