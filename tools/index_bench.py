"""Device time of the index grown from an encode call's slots (ulcx_index_slots_dev) beside the serial walk of the same blocks
packed (ulcx_index_packed_dev): hipEvents around each call on the stream it runs on, the two forms alternating in one
process, a warm-up, then --steps timed calls each.

    python tools/index_bench.py [--steps N] [--warmup W] [--out FILE]

(a) 64 rows x 4000 blocks of stereo 2048 (few long streams: the packed walk runs 64 lanes, 4000 blocks each in series);
(b) 4096 rows x 32 blocks (the headline batch; an index call behind every encode call), beside the VBR encode call that
    produced the slots.
Both forms index the same blocks, and the two indexes are compared entry for entry before anything is timed.  Each timed
slot-form call is begin + append (a fresh index of the whole buffer), the packed call its one kernel.
One JSON line per shape, each with the library's build revision; appended to --out (default profiles/index_slots_bench.txt)."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fns, steps, warmup, torch):
    """fns: {label: call}; the forms alternate call by call, each between two events on the null stream.  -> {label: [ms]}"""
    res = {k: [] for k in fns}
    for i in range(warmup + steps):
        for label, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                res[label].append(e0.elapsed_time(e1))
    return res


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls": len(v)}


def shape(a, emit, torch, ulc_amd, synth_pcm, dev, what, B, K, tile, with_encode):
    """B streams of K encoded blocks, each stream's blocks repeated `tile` times (blocks parse independently): B rows x K * tile blocks."""
    bs, ch, rate = 2048, 2, 44100
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    slot = enc.slot
    d_slots = torch.zeros((B, K, slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((B, K), dtype=torch.int32, device=dev)

    def encode():
        enc.encode_dev(d_pcm.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    encode()
    torch.cuda.synchronize()
    L = K * tile
    if tile > 1:
        d_all, d_allbits = d_slots.repeat(1, tile, 1).contiguous(), d_bits.repeat(1, tile).contiguous()
    else:
        d_all, d_allbits = d_slots, d_bits
    stride = (int(((d_allbits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    d_pay = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(B, dtype=torch.int32, device=dev)
    assert ulc_amd.lib().ulcx_pack_streams_dev(0, B, L, slot, d_all.data_ptr(), d_allbits.data_ptr(), d_pay.data_ptr(), stride,
                                               d_nb.data_ptr(), None, None) == 0
    dec = ulc_amd.BatchDecoder(B, ch, bs, 2)
    one = ulc_amd.BatchDecoder(1, ch, bs, 2)                 # the slot form takes its row count from the call
    d_idx = torch.zeros((B, L + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_pidx = torch.zeros((B, L + 1, 2), dtype=torch.int32, device=dev)
    d_pcnt = torch.zeros(B, dtype=torch.int32, device=dev)

    def slots():
        one.index_begin_dev(B, d_idx.data_ptr(), L + 1, d_cnt.data_ptr())
        one.index_slots_dev(B, d_all.data_ptr(), slot, d_allbits.data_ptr(), L, d_idx.data_ptr(), L + 1, d_cnt.data_ptr())

    def packed():
        dec.index_packed_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), L, d_pidx.data_ptr(), d_pcnt.data_ptr())

    slots(); packed()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_idx, d_pidx)) and bool(torch.equal(d_cnt, d_pcnt)) and int(d_cnt.min().item()) == L
    fns = {"index_slots": slots, "index_packed": packed}
    if with_encode:
        fns["encode_vbr50"] = encode
    r = timed(fns, a.steps, a.warmup, torch)
    line = {"what": what, "rows": B, "blocks": L, "indexes_equal": same,
            "index_slots": stats(r["index_slots"]), "index_packed": stats(r["index_packed"]),
            "packed_over_slots": round(float(np.median(r["index_packed"]) / np.median(r["index_slots"])), 2)}
    if with_encode:
        line["encode_vbr50_call"] = stats(r["encode_vbr50"])
        line["slots_over_encode"] = round(float(np.median(r["index_slots"]) / np.median(r["encode_vbr50"])), 4)
    emit(line)
    enc.close(); dec.close(); one.close()
    assert same, "the two indexes differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of a,b; default: both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_slots_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    out = open(a.out, "a")

    def emit(d):
        d["build"] = rev
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    only = set(a.only.split(",")) if a.only else set("ab")
    if "a" in only:
        shape(a, emit, torch, ulc_amd, synth_pcm, dev, "(a) 64 rows x 4000 blocks of stereo 2048: index from slots / serial walk of the packed payload (device time, hipEvents)",
              64, 40, 100, False)
    if "b" in only:
        shape(a, emit, torch, ulc_amd, synth_pcm, dev, "(b) 4096 rows x 32 blocks of stereo 2048: index from slots / serial walk of the packed payload / the VBR 50 encode call (device time, hipEvents)",
              4096, 32, 1, True)
    out.close()


if __name__ == "__main__":
    main()
