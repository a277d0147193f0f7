"""Wall clock of crop calls on a ragged corpus (ulcx_decode_crops_ragged_dev) beside the strided call on the same rows
(ulcx_decode_crops_dev on the strided copy of the corpus): synchronised calls on device buffers, 20 timed calls per form after a
warm-up, the forms alternating in one process (tools/crops_bench.py's pattern); outputs compared bit for bit first.

    python tools/crops_ragged_bench.py [--steps N] [--warmup W] [--out FILE]

The corpus: 64 files of stereo 2048 whose block counts are spread geometrically from 8 to 4096 (16 distinct encoded streams of 40
blocks, a file's blocks taken from its stream round and round).  4096 rows x 31 blocks, random file, random start.
(a) the crop call in both layouts and the HBM bytes of both.  The yardstick is the strided call in the same process: the ragged
    call reads two offsets per table where the strided one multiplies, and launches the same synthesis, so its median should lie
    inside the strided call's own min-max spread over the run: `ragged_median_within_strided_spread`.
(b) the one-off index of the corpus: ulcx_index_packed_ragged_dev beside ulcx_index_packed_rows_dev on the strided copy (one lane
    per file in both: a wave waits for its longest file).
One JSON line per measurement, each with the library's build revision; appended to --out (default profiles/crops_ragged_bench.txt)."""
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

PAD = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_ragged_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    out = open(a.out, "a")
    sync = torch.cuda.synchronize

    def emit(d):
        d["ulcx_build_rev"] = rev
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    bs, ch, rate, F, K0, N, n = 2048, 2, 44100, 64, 40, 31, 4096
    blocks = np.unique(np.round(np.geomspace(8, 4096, F)).astype(np.int64))
    assert blocks.size == F and blocks[0] == 8 and blocks[-1] == 4096, blocks
    # 16 distinct synthetic streams encoded at VBR 50; file f is blocks 0, 1, .. of stream f % 16, round and round
    base = np.stack([synth_pcm(s, K0 * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    enc = ulc_amd.BatchEncoder(16, ch, bs, rate, K0)
    slots, bits, _, _ = enc.encode(base, ulc_amd.MODE_VBR, 50.0)
    enc.close()
    nb = (bits.astype(np.int64) + 7) // 8
    pays = []
    for f in range(F):
        s = f % 16
        one = [slots[s, k, :nb[s, k]] for k in range(K0)]
        pays.append(np.concatenate([one[k % K0] for k in range(int(blocks[f]))]))
    sizes = np.array([p.size for p in pays], np.int64)
    # the ragged layout and its strided copy
    poffs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ioffs = np.concatenate([[0], np.cumsum(blocks + 1)]).astype(np.int64)
    ragged = np.zeros(int(poffs[-1]) + PAD, np.uint8)
    stride, istride = (int(sizes.max()) + PAD + 15) & ~15, int(blocks.max()) + 1
    strided = np.zeros((F, stride), np.uint8)
    for f, p in enumerate(pays):
        ragged[poffs[f]:poffs[f + 1]] = p
        strided[f, :p.size] = p
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    r_pay, r_po, r_io = t(ragged), t(poffs), t(ioffs)
    r_idx = torch.zeros((int(ioffs[-1]), 2), dtype=torch.int32, device=dev)
    r_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    s_pay, s_nb = t(strided), t(sizes.astype(np.int32))
    s_idx = torch.zeros((F, istride, 2), dtype=torch.int32, device=dev)
    s_cnt = torch.zeros(F, dtype=torch.int32, device=dev)
    dec = ulc_amd.BatchDecoder(n, ch, bs, N + 1)

    # (b) first: the index both crop calls need
    def index_ragged():
        dec.index_packed_ragged_dev(F, r_pay.data_ptr(), r_pay.numel(), r_po.data_ptr(), r_idx.data_ptr(), r_idx.shape[0], r_io.data_ptr(), r_cnt.data_ptr())

    def index_strided():
        dec.index_packed_rows_dev(F, s_pay.data_ptr(), stride, s_nb.data_ptr(), istride - 1, s_idx.data_ptr(), s_cnt.data_ptr())

    index_ragged(); index_strided(); sync()
    cnt = r_cnt.cpu().numpy()
    assert np.array_equal(cnt, blocks), "every file has its whole blocks"
    rows_equal = bool(torch.equal(r_cnt, s_cnt) and all(torch.equal(r_idx[ioffs[f]:ioffs[f + 1]], s_idx[f, :blocks[f] + 1]) for f in range(F)))
    ri = timed({"ragged": index_ragged, "strided": index_strided}, a.steps, a.warmup, sync)
    emit({"what": "(b) one-off index of 64 files of stereo 2048, 8 .. 4096 blocks: ulcx_index_packed_ragged_dev beside ulcx_index_packed_rows_dev "
                  "on the strided copy (wall clock)",
          "index_ragged": stats(ri["ragged"]), "index_strided": stats(ri["strided"]), "rows_equal": rows_equal, "blocks_indexed": int(blocks.sum())})

    # (a) the crop call
    rng = np.random.default_rng(3)
    fno = rng.integers(0, F, n)
    files = t(fno.astype(np.int32))
    first = t(rng.integers(0, np.maximum(blocks[fno] - N, 0) + 1).astype(np.int32))
    outs = {k: torch.zeros((n, N, bs, ch), dtype=torch.float32, device=dev) for k in ("ragged", "strided")}
    obits = {k: torch.zeros((n, N), dtype=torch.int32, device=dev) for k in outs}
    stages = {k: ([], []) for k in outs}

    def note(k):
        sync()
        st = dec.stage_ms()
        stages[k][0].append(st["k_dscan"]); stages[k][1].append(st["k_dsyn"])

    def crops_ragged():
        dec.decode_crops_ragged_dev(F, r_pay.data_ptr(), r_pay.numel(), r_po.data_ptr(), r_idx.data_ptr(), r_idx.shape[0], r_io.data_ptr(), r_cnt.data_ptr(),
                                    n, files.data_ptr(), first.data_ptr(), 0, N, outs["ragged"].data_ptr(), obits["ragged"].data_ptr())
        note("ragged")

    def crops_strided():
        dec.decode_crops_dev(F, s_pay.data_ptr(), stride, s_nb.data_ptr(), s_idx.data_ptr(), istride, s_cnt.data_ptr(), n, files.data_ptr(),
                             first.data_ptr(), 0, N, outs["strided"].data_ptr(), obits["strided"].data_ptr())
        note("strided")

    crops_ragged(); crops_strided()
    same = bool(torch.equal(outs["ragged"].view(torch.int32), outs["strided"].view(torch.int32)) and torch.equal(obits["ragged"], obits["strided"]))
    assert same, "the ragged and the strided call differ"
    decoded = int((obits["ragged"] > 0).sum().item())
    stages = {k: ([], []) for k in outs}
    r = timed({"ragged": crops_ragged, "strided": crops_strided}, a.steps, a.warmup, sync)
    sr, ss = stats(r["ragged"]), stats(r["strided"])
    emit({"what": "(a) 4096 rows x 31 blocks of stereo 2048 from a corpus of 64 files of 8 .. 4096 blocks: ragged crop call beside the strided call "
                  "on the strided copy (wall clock; scan / syn: device time of the stages)",
          "ragged": sr, "strided": ss, "ragged_median_within_strided_spread": bool(ss["min_ms"] <= sr["median_ms"] <= ss["max_ms"]),
          "ragged_median_over_strided_median": round(sr["median_ms"] / ss["median_ms"], 4),
          "ragged_scan": stats(stages["ragged"][0][a.warmup:]), "ragged_syn": stats(stages["ragged"][1][a.warmup:]),
          "strided_scan": stats(stages["strided"][0][a.warmup:]), "strided_syn": stats(stages["strided"][1][a.warmup:]),
          "outputs_equal": same, "blocks_decoded_of_rows_x_31": [decoded, n * N], "cut_of_last_call": list(dec.last_cut()),
          "hbm_bytes_ragged": nbytes(r_pay, r_po, r_idx, r_io, r_cnt), "hbm_bytes_strided": nbytes(s_pay, s_nb, s_idx, s_cnt)})
    dec.close()
    out.close()


if __name__ == "__main__":
    main()
