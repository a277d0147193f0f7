"""Wall clock of the ladder call (ulcx_encode_dev_ladder) against the same rungs as separate calls on separate encoders:
synchronised calls, device buffers, all forms alternating in one process, two rounds.

    python tools/ladder_bench.py [--steps N] [--warmup W] [--shapes headline,wswitch_4096]

Shapes: the headline shape (4096 stereo streams x 32 blocks of 2048 at 44.1 kHz) and the window-switching configuration's
(2048 streams x 16 blocks of 4096 at 48 kHz).  Forms:
    plain       ulcx_encode_dev, VBR 50                          ladder1     the same as a one-rung ladder
    ladder2/4   scalar VBR rungs (qualities 30, 50 / 30, 50, 70, 90)          sep2/4      the same rungs, one plain call each
    ladder_mix  VBR 50, CBR 64, ABR 96 at 0.3, one per-stream table           sep_mix     the same, one call each
A sample of a sep form is the sum of its calls, each synchronised.  One JSON line per shape: median and min/max ms of every
form, the plain call's spread, the ratios ladder / separate, the cost of an extra VBR rung (ladder2 - ladder1) beside that rung
as a call of its own, the time saved per rung behind the first, and outputs_equal - every rung of every ladder compared with its
separate call (sizes, and the bytes the sizes cover)."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

VBR4 = [(0, 30.0, 0.0), (0, 50.0, 0.0), (0, 70.0, 0.0), (0, 90.0, 0.0)]
TABLE = [(-50.0, 0.0), (32.0, 0.0), (64.0, 0.35), (-80.0, 0.0), (96.0, 0.0), (128.0, 0.5), (-20.0, 0.0), (48.0, 0.2)]


def run(name, B, K, bs, rate, steps, warmup):
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    ch = 2
    dev = torch.device("cuda:0")
    # a few distinct synthetic streams tiled over the batch (the content only has to be realistic, not unique)
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    d_table = torch.tensor([TABLE[s % len(TABLE)] for s in range(B)], dtype=torch.float32, device=dev)
    lad = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    sep = [ulc_amd.BatchEncoder(B, ch, bs, rate, K) for _ in range(4)]
    for e in [lad] + sep:
        e.set_timing(False)
    slot = lad.slot
    l_out = torch.zeros((4, B, K, slot), dtype=torch.uint8, device=dev)
    l_bits = torch.zeros((4, B, K), dtype=torch.int32, device=dev)
    s_out, s_bits = torch.zeros_like(l_out), torch.zeros_like(l_bits)
    st = torch.cuda.current_stream(dev)
    mix = [(0, 50.0, 0.0), (1, 64.0, 0.0), (2, 96.0, 0.3), d_table.data_ptr()]

    def ladder(rungs):
        def fn():
            lad.encode_dev_ladder(rungs, d_pcm.data_ptr(), K, l_out.data_ptr(), l_bits.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
        return fn

    def one(r, g):
        if isinstance(g, tuple):
            sep[r].encode_dev(d_pcm.data_ptr(), K, s_out[r].data_ptr(), s_bits[r].data_ptr(), mode=g[0], p0=g[1], p1=g[2], stream=st.cuda_stream)
        else:
            sep[r].encode_dev_rates(g, d_pcm.data_ptr(), K, s_out[r].data_ptr(), s_bits[r].data_ptr(), stream=st.cuda_stream)
        st.synchronize()

    def separate(rungs):
        def fn():
            for r, g in enumerate(rungs):
                one(r, g)
        return fn

    forms = [("plain", separate(VBR4[1:2])), ("ladder1", ladder(VBR4[1:2])), ("ladder2", ladder(VBR4[:2])), ("sep2", separate(VBR4[:2])),
             ("ladder4", ladder(VBR4)), ("sep4", separate(VBR4)), ("ladder_mix", ladder(mix)), ("sep_mix", separate(mix))]
    res = {label: [] for label, _ in forms}
    for rep in range(2):
        for label, fn in forms:
            for e in [lad] + sep:
                e.reset()                                          # (every form times the same blocks of the same streams)
            for _ in range(warmup):
                fn()
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()
                res[label].append((time.perf_counter() - t0) * 1e3)

    # every rung of every ladder against its separate call, from the same state
    def equal(rungs):
        for e in [lad] + sep:
            e.reset()
        ladder(rungs)()
        separate(rungs)()
        ok = True
        col = torch.arange(slot, device=dev)
        for r in range(len(rungs)):
            ok = ok and bool(torch.equal(l_bits[r], s_bits[r]))
            covered = col[None, None, :] < (s_bits[r] // 8)[:, :, None]
            ok = ok and bool(((l_out[r] == s_out[r]) | ~covered).all())
            del covered
        return ok and bool((l_bits[:len(rungs)] > 0).all())
    same = all(equal(r) for r in (VBR4[1:2], VBR4[:2], VBR4, mix))
    for e in [lad] + sep:
        e.close()
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"shape": name, "streams": B, "blocks": K, "block_size": bs, "rate_hz": rate}
    for k, v in res.items():
        out[k + "_ms"] = round(med[k], 3)
        out[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    out.update({"plain_spread_ms": round(max(res["plain"]) - min(res["plain"]), 3),
                "ladder1_minus_plain_ms": round(med["ladder1"] - med["plain"], 3),
                "ratio_ladder2": round(med["ladder2"] / med["sep2"], 4), "ratio_ladder4": round(med["ladder4"] / med["sep4"], 4),
                "ratio_ladder_mix": round(med["ladder_mix"] / med["sep_mix"], 4),
                # what the quality-30 rung adds to the quality-50 call, against that rung as a call of its own
                "extra_vbr_rung_ms": round(med["ladder2"] - med["ladder1"], 3), "that_rung_alone_ms": round(med["sep2"] - med["plain"], 3),
                "saved_per_extra_rung_ms": {k: round((med["sep" + k] - med["ladder" + k]) / n, 3) for k, n in (("2", 1), ("4", 3), ("_mix", 3))},
                "steps": 2 * steps, "outputs_equal": same, "build": ulc_amd.build_rev()})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per form and round (two rounds, forms alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="headline,wswitch_4096")
    a = ap.parse_args()
    shapes = {"headline": (4096, 32, 2048, 44100), "wswitch_4096": (2048, 16, 4096, 48000)}
    for name in a.shapes.split(","):
        run(name, *shapes[name], a.steps, a.warmup)


if __name__ == "__main__":
    main()
