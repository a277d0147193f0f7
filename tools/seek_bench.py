"""Wall clock of the block index and of range decodes (ulcx_index_packed_dev / ulcx_decode_range_dev) beside the packed
calls they replace: synchronised calls on device buffers, 20 timed calls per form after a warm-up, the forms alternating
in one process.

    python tools/seek_bench.py [--steps N] [--warmup W] [--out FILE]

(a) index of 4096 stereo payloads of 32 blocks of 2048, beside the scan stage of a packed call on the same payloads;
(b) a range call of 31 blocks from that index (from block 0: the same 31 blocks; from block 1: with the block in front),
    beside a packed call of 31 blocks;
(c) 64 streams of 4096 blocks: one range call of 31 blocks at block 4000, beside the 126 packed calls of 32 blocks that get
    there from block 0 (and the index of the 4096 blocks, built once).
(d) a range call of 7 blocks of 1600 streams (one whole round of an MI355X's 1536 resident workgroups + 64 streams) under
    the three launch plans: the cut of the last round (the default for range calls), the even cut (ULCX_RANGE_CUT=even),
    one workgroup per stream (ULCX_DSYN_SPLIT=0).
One JSON line per measurement, each with the library's build revision; appended to --out (default profiles/seek_bench.txt)."""
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
    """fns: {label: (prepare or None, call)}; the forms alternate call by call.  -> {label: [ms]}"""
    res = {k: [] for k in fns}
    for i in range(warmup + steps):
        for label, (prep, fn) in fns.items():
            if prep:
                prep()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                res[label].append((time.perf_counter() - t0) * 1e3)
    return res


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls": len(v)}


def plans_1600x7(a, emit, torch, ulc_amd, synth_pcm, dev):
    """(d): the same range call on three decoders created under different plan switches, alternating call by call."""
    sync = torch.cuda.synchronize
    bs, ch, rate, B, K, N = 2048, 2, 44100, 1600, 40, 7
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    d_slots = torch.zeros((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((B, K), dtype=torch.int32, device=dev)
    enc.encode_dev(d_pcm.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    sync()
    stride = (int(((d_bits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    d_pay = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(B, dtype=torch.int32, device=dev)
    assert ulc_amd.lib().ulcx_pack_streams_dev(0, B, K, enc.slot, d_slots.data_ptr(), d_bits.data_ptr(), d_pay.data_ptr(), stride,
                                               d_nb.data_ptr(), None, None) == 0
    sync()
    enc.close()
    d_idx = torch.zeros((B, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    first = torch.from_numpy(np.random.default_rng(3).integers(0, K - N + 1, B).astype(np.int32)).to(dev)
    d_ob = torch.zeros((B, N), dtype=torch.int32, device=dev)
    decs, outs, fns, syn = {}, {}, {}, {}
    for label, env in (("tail_cut", {}), ("even_cut", {"ULCX_RANGE_CUT": "even"}), ("whole_streams", {"ULCX_DSYN_SPLIT": "0"})):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        decs[label] = ulc_amd.BatchDecoder(B, ch, bs, N + 1)          # (the switches are read when a decoder is created)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        outs[label] = torch.zeros((B, N, bs, ch), dtype=torch.float32, device=dev)
        syn[label] = []

        def call(label=label):
            d = decs[label]
            d.decode_range_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), first.data_ptr(), N,
                               outs[label].data_ptr(), d_ob.data_ptr())
            sync()
            syn[label].append(d.stage_ms()["k_dsyn"])
        fns[label] = (None, call)
    decs["tail_cut"].index_packed_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())
    sync()
    r = timed(fns, a.steps, a.warmup, sync)
    same = all(bool(torch.equal(outs["tail_cut"].view(torch.int32), o.view(torch.int32))) for o in outs.values())
    line = {"what": "(d) range call of 7 blocks of 1600 streams under three launch plans (wall clock; syn: device time of the synthesis stage)",
            "outputs_equal": same}
    for label in fns:
        line[label] = stats(r[label]); line[label + "_syn"] = stats(syn[label][a.warmup:]); line[label + "_cut"] = list(decs[label].last_cut())
        decs[label].close()
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list of a,b,c,d (a and b run together); default: all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seek_bench.txt"))
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

    sync = torch.cuda.synchronize
    only = set(a.only.split(",")) if a.only else set("abcd")
    if "d" in only:
        plans_1600x7(a, emit, torch, ulc_amd, synth_pcm, dev)
    if not (only & set("abc")):
        out.close()
        return
    bs, ch, rate, B, K = 2048, 2, 44100, 4096, 32
    # a few distinct synthetic streams tiled over the batch, encoded at VBR 50 and packed as the tool writes them
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    d_slots = torch.zeros((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((B, K), dtype=torch.int32, device=dev)
    enc.encode_dev(d_pcm.data_ptr(), K, d_slots.data_ptr(), d_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
    sync()
    stride = (int(((d_bits + 7) // 8).sum(dim=1).max().item()) + 64 + 15) & ~15
    d_pay = torch.zeros((B, stride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(B, dtype=torch.int32, device=dev)
    rc = ulc_amd.lib().ulcx_pack_streams_dev(0, B, K, enc.slot, d_slots.data_ptr(), d_bits.data_ptr(), d_pay.data_ptr(), stride,
                                             d_nb.data_ptr(), None, None)
    assert rc == 0
    sync()
    enc.close()
    del d_slots, d_pcm

    dec = ulc_amd.BatchDecoder(B, ch, bs, K)
    d_idx = torch.zeros((B, K + 1, 2), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_out = torch.zeros((B, K, bs, ch), dtype=torch.float32, device=dev)
    d_ob = torch.zeros((B, K), dtype=torch.int32, device=dev)
    first0 = torch.zeros(B, dtype=torch.int32, device=dev)
    first1 = torch.ones(B, dtype=torch.int32, device=dev)
    scan_ms, syn_ms = [], []

    def index():
        dec.index_packed_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), K, d_idx.data_ptr(), d_cnt.data_ptr())

    def packed(n, stages=None):
        def f():
            dec.decode_packed_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), n, d_out.data_ptr(), d_ob.data_ptr())
            if stages is not None:
                sync()
                st = dec.stage_ms()
                stages[0].append(st["k_dscan"]); stages[1].append(st["k_dsyn"])
        return f

    def ranged(first, n, stages=None):
        def f():
            dec.decode_range_dev(d_pay.data_ptr(), stride, d_nb.data_ptr(), d_idx.data_ptr(), K + 1, d_cnt.data_ptr(), first.data_ptr(), n,
                                 d_out.data_ptr(), d_ob.data_ptr())
            if stages is not None:
                sync()
                st = dec.stage_ms()
                stages[0].append(st["k_dscan"]); stages[1].append(st["k_dsyn"])
        return f

    index(); sync()
    assert int(d_cnt.min().item()) == K, "every stream has 32 whole blocks"
    # (a) the index beside a packed call's scan stage (device time of the stage, hipEvents)
    r = timed({"index": (None, index), "packed32": (dec.reset, packed(K, (scan_ms, syn_ms)))}, a.steps, a.warmup, sync)
    emit({"what": "(a) index of 4096 x 32 blocks of 2048 (wall clock) beside the packed call's scan stage (device time)",
          "index": stats(r["index"]), "packed_call_32": stats(r["packed32"]), "packed_scan_stage": stats(scan_ms[a.warmup:]),
          "packed_syn_stage": stats(syn_ms[a.warmup:])})
    # (b) 31 blocks: by range from block 0 (the same blocks as the packed call), by range from block 1 (with the block in front), packed
    st0, st1, stp = ([], []), ([], []), ([], [])
    r = timed({"range0": (None, ranged(first0, K - 1, st0)), "range1": (None, ranged(first1, K - 1, st1)),
               "packed31": (dec.reset, packed(K - 1, stp))}, a.steps, a.warmup, sync)
    emit({"what": "(b) 31 blocks of 4096 streams: range call from block 0 / from block 1, packed call (wall clock; stages: device time)",
          "range_from_0": stats(r["range0"]), "range_from_1": stats(r["range1"]), "packed": stats(r["packed31"]),
          "range_from_0_scan": stats(st0[0][a.warmup:]), "range_from_0_syn": stats(st0[1][a.warmup:]),
          "range_from_1_scan": stats(st1[0][a.warmup:]), "range_from_1_syn": stats(st1[1][a.warmup:]),
          "packed_scan": stats(stp[0][a.warmup:]), "packed_syn": stats(stp[1][a.warmup:]), "cut_of_last_call": list(dec.last_cut())})
    dec.close()
    if "c" not in only:
        out.close()
        return

    # (c) 64 long streams: each payload of (a) 128 times over = 4096 blocks
    B2, REP, NBLK, AT, N = 64, 128, 4096, 4000, 31
    pay = d_pay[:B2].cpu().numpy(); nb = d_nb[:B2].cpu().numpy()
    stride2 = (int(nb.max()) * REP + 64 + 15) & ~15
    host = np.zeros((B2, stride2), np.uint8)
    for s in range(B2):
        host[s, :int(nb[s]) * REP] = np.tile(pay[s, :int(nb[s])], REP)
    d_pay2 = torch.from_numpy(host).to(dev)
    d_nb2 = torch.from_numpy((nb.astype(np.int64) * REP).astype(np.int32)).to(dev)
    dec = ulc_amd.BatchDecoder(B2, ch, bs, K)
    d_idx2 = torch.zeros((B2, NBLK + 1, 2), dtype=torch.int32, device=dev)
    d_cnt2 = torch.zeros(B2, dtype=torch.int32, device=dev)
    d_first = torch.full((B2,), AT, dtype=torch.int32, device=dev)
    d_seq = torch.zeros((B2, K, bs, ch), dtype=torch.float32, device=dev)
    d_rng = torch.zeros((B2, N, bs, ch), dtype=torch.float32, device=dev)

    def index2():
        dec.index_packed_dev(d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), NBLK, d_idx2.data_ptr(), d_cnt2.data_ptr())

    def seek():
        dec.decode_range_dev(d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), d_idx2.data_ptr(), NBLK + 1, d_cnt2.data_ptr(), d_first.data_ptr(), N,
                             d_rng.data_ptr(), d_ob.data_ptr())

    def walk():
        for _ in range((AT + N + K - 1) // K):                    # 126 calls of 32 blocks: blocks 0 .. 4031
            dec.decode_packed_dev(d_pay2.data_ptr(), stride2, d_nb2.data_ptr(), K, d_seq.data_ptr(), d_ob.data_ptr())

    index2(); sync()
    assert int(d_cnt2.min().item()) == NBLK
    r = timed({"index": (None, index2), "range": (None, seek), "packed_walk": (dec.reset, walk)}, a.steps, a.warmup, sync)
    # the walk's last call holds blocks 4000 .. 4031: the range call's 31 blocks are its first 31
    same = bool(torch.equal(d_seq[:, :N].view(torch.int32), d_rng.view(torch.int32)))
    emit({"what": "(c) 64 streams x 4096 blocks: index (once per file), one range call of 31 blocks at block 4000, the 126 packed calls that reach it",
          "index_4096_blocks": stats(r["index"]), "range_at_4000": stats(r["range"]), "packed_walk_126_calls": stats(r["packed_walk"]),
          "range_equals_walk": same})
    dec.close()
    out.close()


if __name__ == "__main__":
    main()
