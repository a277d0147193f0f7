"""Wall clock of crop calls (ulcx_decode_crops_dev) beside the range call they replace: synchronised calls on device buffers,
20 timed calls per form after a warm-up, the forms alternating in one process (tools/seek_bench.py's pattern).

    python tools/crops_bench.py [--steps N] [--warmup W] [--only a,b] [--out FILE]

(a) 4096 rows x 31 blocks of stereo 2048 drawn from a corpus of 64 files of 40 blocks (random file, random start), beside
    ulcx_decode_range_dev on the same rows with every row's payload and index copied out: the corpus replicated to 4096 streams.
    The crop call does the range call's work plus a file number and the row's index entries per lane, so its median should lie
    inside the range call's own min-max spread over the run: `crop_median_within_range_spread`.
(b) 64 rows x 31 blocks at random starts of a corpus of 64 files x 4096 blocks (random file per row), beside the range call of a
    64-stream decoder on the corpus itself from the same starts (row i = file i: what a range call can do without copies).
For both: the HBM bytes of corpus + index, and of the replicated form (one payload and index row per row of the call).
One JSON line per measurement, each with the library's build revision; appended to --out (default profiles/crops_bench.txt)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fns, steps, warmup, sync):
    """fns: {label: call}; the forms alternate call by call.  -> {label: [ms]}"""
    res = {k: [] for k in fns}
    for i in range(warmup + steps):
        for label, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                res[label].append((time.perf_counter() - t0) * 1e3)
    return res


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls": len(v)}


def nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of a,b; default: both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    out = open(a.out, "a")
    sync = torch.cuda.synchronize
    only = set(a.only.split(",")) if a.only else set("ab")

    def emit(d):
        d["ulcx_build_rev"] = rev
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    bs, ch, rate, F, K, N = 2048, 2, 44100, 64, 40, 31
    # the corpus: 16 distinct synthetic streams tiled to 64 files, encoded at VBR 50 and packed as the tool writes them
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

    if "a" in only:
        n = 4096
        dec = ulc_amd.BatchDecoder(n, ch, bs, N + 1)
        d_idx = torch.zeros((F, K + 1, 2), dtype=torch.int32, device=dev)
        d_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
        dec.index_packed_rows_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
        sync()
        assert int(d_cnt.min().item()) == K, "every file has 40 whole blocks"
        rng = np.random.default_rng(3)
        files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
        first = torch.from_numpy(rng.integers(0, K - N + 1, n).astype(np.int32)).to(dev)
        pick = files.long()
        r_pay, r_nb, r_idx, r_cnt = d_pay[pick].contiguous(), d_nb[pick].contiguous(), d_idx[pick].contiguous(), d_cnt[pick].contiguous()
        outs = {k: torch.zeros((n, N, bs, ch), dtype=torch.float32, device=dev) for k in ("crops", "range")}
        obits = {k: torch.zeros((n, N), dtype=torch.int32, device=dev) for k in outs}
        stages = {k: ([], []) for k in outs}

        def note(k):
            sync()
            st = dec.stage_ms()
            stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])

        def crops():
            dec.decode_crops_dev(F, d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), n, files.data_ptr(),
                                 first.data_ptr(), 0, N, outs["crops"].data_ptr(), obits["crops"].data_ptr())
            note("crops")

        def ranged():
            dec.decode_range_dev(r_pay.data_ptr(), stride, r_nb.data_ptr(), r_idx.data_ptr(), K + 1, r_cnt.data_ptr(), first.data_ptr(), N,
                                 outs["range"].data_ptr(), obits["range"].data_ptr())
            note("range")

        r = timed({"crops": crops, "range": ranged}, a.steps, a.warmup, sync)
        same = bool(torch.equal(outs["crops"].view(torch.int32), outs["range"].view(torch.int32)) and torch.equal(obits["crops"], obits["range"]))
        sc, sr = stats(r["crops"]), stats(r["range"])
        emit({"what": "(a) 4096 rows x 31 blocks of stereo 2048 from a 64-file corpus: crop call beside the range call on the replicated corpus "
                      "(wall clock; scan / syn: device time of the stages)",
              "crops": sc, "range_replicated": sr, "crop_median_within_range_spread": bool(sr["min_ms"] <= sc["median_ms"] <= sr["max_ms"]),
              "crops_scan": stats(stages["crops"][0][a.warmup:]), "crops_syn": stats(stages["crops"][1][a.warmup:]),
              "range_scan": stats(stages["range"][0][a.warmup:]), "range_syn": stats(stages["range"][1][a.warmup:]),
              "outputs_equal": same, "cut_of_last_call": list(dec.last_cut()),
              "hbm_bytes_corpus_and_index": nbytes(d_pay, d_nb, d_idx, d_cnt), "hbm_bytes_replicated": nbytes(r_pay, r_nb, r_idx, r_cnt)})
        dec.close()
        del r_pay, r_idx, outs

    if "b" in only:
        # 64 long files: each payload 103 times over, indexed up to 4096 blocks
        REP, NBLK, n = 103, 4096, 64
        pay = d_pay.cpu().numpy(); nb = d_nb.cpu().numpy()
        stride2 = (int(nb.max()) * REP + 64 + 15) & ~15
        host = np.zeros((F, stride2), np.uint8)
        for s in range(F):
            host[s, :int(nb[s]) * REP] = np.tile(pay[s, :int(nb[s])], REP)
        d_pay2 = torch.from_numpy(host).to(dev)
        d_nb2 = torch.from_numpy((nb.astype(np.int64) * REP).astype(np.int32)).to(dev)
        dec = ulc_amd.BatchDecoder(n, ch, bs, N + 1)
        d_idx2 = torch.zeros((F, NBLK + 1, 2), dtype=torch.int32, device=dev)
        d_cnt2 = torch.zeros(F, dtype=torch.int32, device=dev)
        dec.index_packed_rows_dev(F, d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), NBLK, d_idx2.data_ptr(), d_cnt2.data_ptr())
        sync()
        assert int(d_cnt2.min().item()) == NBLK
        rng = np.random.default_rng(4)
        files = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).to(dev)
        ident = torch.arange(F, dtype=torch.int32, device=dev)
        first = torch.from_numpy(rng.integers(0, NBLK - N + 1, n).astype(np.int32)).to(dev)
        o = {k: torch.zeros((n, N, bs, ch), dtype=torch.float32, device=dev) for k in ("crops", "crops_identity", "range")}
        ob = torch.zeros((n, N), dtype=torch.int32, device=dev)

        def crop(which, label):
            return lambda: dec.decode_crops_dev(F, d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), d_idx2.data_ptr(), NBLK + 1, d_cnt2.data_ptr(), n,
                                                which.data_ptr(), first.data_ptr(), 0, N, o[label].data_ptr(), ob.data_ptr())

        def ranged():
            dec.decode_range_dev(d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), d_idx2.data_ptr(), NBLK + 1, d_cnt2.data_ptr(), first.data_ptr(), N,
                                 o["range"].data_ptr(), ob.data_ptr())

        r = timed({"crops": crop(files, "crops"), "crops_identity": crop(ident, "crops_identity"), "range": ranged}, a.steps, a.warmup, sync)
        same = bool(torch.equal(o["crops_identity"].view(torch.int32), o["range"].view(torch.int32)))
        per_row = nbytes(d_pay2[0], d_nb2[0], d_idx2[0], d_cnt2[0])
        emit({"what": "(b) 64 rows x 31 blocks at random starts of a corpus of 64 files x 4096 blocks: crop call (random file per row; row i = file i) "
                      "beside the range call of the corpus itself (wall clock)",
              "crops_random_files": stats(r["crops"]), "crops_identity": stats(r["crops_identity"]), "range_identity": stats(r["range"]),
              "identity_outputs_equal": same, "distinct_files_named": int(files.unique().numel()),
              "hbm_bytes_corpus_and_index": nbytes(d_pay2, d_nb2, d_idx2, d_cnt2), "hbm_bytes_replicated": per_row * n})
        dec.close()
    out.close()


if __name__ == "__main__":
    main()
