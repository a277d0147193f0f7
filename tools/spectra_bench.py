"""Wall clock of the spectra call (ulcx_decode_crops_spectra_dev) beside the crop call on the same rows: synchronised calls on
device buffers, 20 timed calls per form after a warm-up, the forms alternating in one process (tools/crops_bench.py's pattern).

    python tools/spectra_bench.py [--steps N] [--warmup W] [--only a,b] [--out FILE]

(a) 4096 rows x 31 blocks of stereo 2048 drawn from a corpus of 64 files of 40 blocks (random file, random start).
(b) 64 rows x 31 blocks at random starts of a corpus of 64 files x 4096 blocks (random file per row).
The forms, per shape:
  spectra     ulcx_decode_crops_spectra_dev, flags 0: [n][2][31][2048] coefficients of the coded mid / side channels
  spectra_lr  the same with ULCX_SPECTRA_LR
  crops       ulcx_decode_crops_dev on the same rows: [n][31][2048][2] samples - the same number of output bytes
The spectra call does strictly less than the crop call (no transform, no windowing, no lapping traffic, no synthesis of the block
in front), so `spectra_median_at_or_below_crops` is the condition; `spectra_over_crops` and `lr_over_spectra` are the medians'
ratios.  walk / expand: device time of the call's two stages (ulcx_decoder_stage_ms: the crop walk; k_dspec, or the synthesis for
the crop call), taken outside the wall-clock loop.  Before anything is timed the spectra call's d_bits is compared with the crop
call's and the LR output with m + s / m - s of the flags-0 output.  One JSON line per shape with the library's build revision,
appended to --out (default profiles/spectra_bench.txt)."""
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
    ap.add_argument("--only", default="", help="comma list of a,b; default: both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    out = open(a.out, "a")
    sync = torch.cuda.synchronize
    only = set(a.only.split(",")) if a.only else set("ab")

    bs, ch, rate, F, K, N = 2048, 2, 44100, 64, 40, 31
    # the corpus of tools/crops_bench.py: 16 distinct synthetic streams tiled to 64 files, encoded at VBR 50 and packed as the tool writes them
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(F) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(F, ch, bs, rate, K)
    d_slots = torch.zeros((F, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((F, K), dtype=torch.int32, device=dev)
    enc.encode_dev(d_pcm.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    sync()
    stride = (int(((d_bits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    d_pay = torch.zeros((F, stride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(F, dtype=torch.int32, device=dev)
    assert ulc_amd.lib().ulcx_pack_streams_dev(0, F, K, enc.slot, d_slots.data_ptr(), d_bits.data_ptr(), d_pay.data_ptr(), stride,
                                               d_nb.data_ptr(), None, None) == 0
    sync()
    enc.close()
    del d_slots, d_pcm

    def shape(what, n, pay, pstride, nb, nblk, seed):
        """One shape: n rows of N blocks at random starts of the F files (pay / nb, nblk blocks each) -> its JSON line."""
        dec = ulc_amd.BatchDecoder(n, ch, bs, N + 1)
        d_idx = torch.zeros((F, nblk + 1, 2), dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
        dec.index_packed_rows_dev(F, pay.data_ptr(), pstride, nb.data_ptr(), nblk, d_idx.data_ptr(), d_cnt.data_ptr())
        sync()
        assert int(d_cnt.min().item()) == nblk, "every file has its whole blocks"
        rng = np.random.default_rng(seed)
        files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
        first = torch.from_numpy(rng.integers(0, nblk - N + 1, n).astype(np.int32)).to(dev)
        coef = {k: torch.zeros((n, ch, N, bs), dtype=torch.float32, device=dev) for k in ("spectra", "spectra_lr")}
        o_crop = torch.zeros((n, N, bs, ch), dtype=torch.float32, device=dev)
        wc = torch.zeros((n, N), dtype=torch.int32, device=dev)
        bits = {k: torch.zeros((n, N), dtype=torch.int32, device=dev) for k in ("spectra", "spectra_lr", "crops")}
        stages = {k: ([], []) for k in bits}

        def spectra(label, flags):
            return lambda: dec.decode_crops_spectra_dev(F, pay.data_ptr(), pstride, nb.data_ptr(), d_idx.data_ptr(), nblk + 1, d_cnt.data_ptr(), n,
                                                        files.data_ptr(), first.data_ptr(), 0, N, flags, coef[label].data_ptr(), wc.data_ptr(),
                                                        bits[label].data_ptr())

        def crops():
            dec.decode_crops_dev(F, pay.data_ptr(), pstride, nb.data_ptr(), d_idx.data_ptr(), nblk + 1, d_cnt.data_ptr(), n, files.data_ptr(),
                                 first.data_ptr(), 0, N, o_crop.data_ptr(), bits["crops"].data_ptr())

        fns = {"spectra": spectra("spectra", 0), "spectra_lr": spectra("spectra_lr", ulc_amd.SPECTRA_LR), "crops": crops}
        for fn in fns.values():
            fn()
        sync()
        ms = coef["spectra"]
        same_bits = bool(torch.equal(bits["spectra"], bits["crops"]) and torch.equal(bits["spectra_lr"], bits["crops"]) and int((bits["crops"] > 0).sum().item()) == n * N)
        lr_is_ms = bool(torch.equal(coef["spectra_lr"][:, 0].view(torch.int32), (ms[:, 0] + ms[:, 1]).view(torch.int32))
                        and torch.equal(coef["spectra_lr"][:, 1].view(torch.int32), (ms[:, 0] - ms[:, 1]).view(torch.int32)))
        r = timed(fns, a.steps, a.warmup, sync)
        for _ in range(a.steps):                            # the stages' device time, outside the wall-clock loop (reading it waits for the device)
            for k, fn in fns.items():
                fn(); sync()
                st = dec.stage_ms()
                stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])
        fns["spectra"](); sync(); cut_spectra = list(dec.last_cut())
        crops(); sync(); cut_crops = list(dec.last_cut())
        s = {k: stats(v) for k, v in r.items()}
        ob = nbytes(coef["spectra"])
        line = {"what": what, "spectra": s["spectra"], "spectra_lr": s["spectra_lr"], "crops": s["crops"],
                "spectra_median_at_or_below_crops": bool(s["spectra"]["median_ms"] <= s["crops"]["median_ms"]),
                "spectra_over_crops": round(s["spectra"]["median_ms"] / s["crops"]["median_ms"], 4),
                "lr_over_spectra": round(s["spectra_lr"]["median_ms"] / s["spectra"]["median_ms"], 4),
                "spectra_walk": stats(stages["spectra"][0]), "spectra_expand": stats(stages["spectra"][1]),
                "spectra_lr_walk": stats(stages["spectra_lr"][0]), "spectra_lr_expand": stats(stages["spectra_lr"][1]),
                "crops_walk": stats(stages["crops"][0]), "crops_syn": stats(stages["crops"][1]),
                "bits_equal_the_crop_calls": same_bits, "lr_is_ms_unmixed": lr_is_ms,
                "output_bytes_spectra": ob, "output_bytes_crops": nbytes(o_crop),
                "spectra_output_GB_per_s": round(ob / (s["spectra"]["median_ms"] * 1e-3) / 1e9, 1),
                "spectra_expand_output_GB_per_s": round(ob / (stats(stages["spectra"][1])["median_ms"] * 1e-3) / 1e9, 1),
                "cut_of_spectra_call": cut_spectra, "cut_of_crop_call": cut_crops, "ulcx_build_rev": rev}
        dec.close()
        text = json.dumps(line)
        print(text, flush=True)
        out.write(text + "\n"); out.flush()

    if "a" in only:
        shape("(a) 4096 rows x 31 blocks of stereo 2048 from a 64-file corpus: the spectra call (flags 0, LR) beside the crop call on the same rows "
              "(wall clock; walk / expand / syn: device time of the stages)", 4096, d_pay, stride, d_nb, K, 3)
    if "b" in only:
        # 64 long files: each payload 103 times over, indexed up to 4096 blocks (tools/crops_bench.py (b))
        REP, NBLK = 103, 4096
        pay = d_pay.cpu().numpy(); nb = d_nb.cpu().numpy()
        stride2 = (int(nb.max()) * REP + 64 + 15) & ~15
        host = np.zeros((F, stride2), np.uint8)
        for s in range(F):
            host[s, :int(nb[s]) * REP] = np.tile(pay[s, :int(nb[s])], REP)
        d_pay2 = torch.from_numpy(host).to(dev)
        d_nb2 = torch.from_numpy((nb.astype(np.int64) * REP).astype(np.int32)).to(dev)
        shape("(b) 64 rows x 31 blocks at random starts of a corpus of 64 files x 4096 blocks (random file per row): the spectra call (flags 0, LR) "
              "beside the crop call on the same rows (wall clock; walk / expand / syn: device time of the stages)", 64, d_pay2, stride2, d_nb2, NBLK, 4)
    out.close()


if __name__ == "__main__":
    main()
