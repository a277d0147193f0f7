"""Wall clock of the stream-slot subset calls against the plain calls on the same object and input: synchronised calls on
device buffers, per-kernel events off (set_timing(False)), the forms alternating in one process.

    python tools/slots_bench.py [--steps N] [--warmup W] [--streams B] [--blocks K] [--out profiles/slots_bench.txt]

At the headline shape (4096 stereo streams x 32 blocks of 2048 at 44.1 kHz, VBR 50), for encode and for decode:
  identity   the subset call over every slot in order against the plain call: what gather + scatter cost
  half       a subset call of B / 2 slots against the plain call of all B: what a caller pays today by feeding silence to the
             absent half
One JSON line per pair (median, min and max ms of each form), printed and appended to --out.  The identity pair also
carries the copy estimate from bytes alone: gather and scatter each read and write every listed slot's state once."""
import argparse
import json
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
COPY_TBPS = 6.3                                            # what a device-to-device copy reaches (profiles/NOTES_r*.md)


def timed(forms, reset, sync, steps, warmup):
    """forms: {label: fn}; two rounds, forms alternating, each from a reset object -> {label: [ms]}"""
    res = {k: [] for k in forms}
    for _ in range(2):
        for label, fn in forms.items():
            reset()
            for _ in range(warmup):
                fn()
            sync()
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()
                sync()
                res[label].append((time.perf_counter() - t0) * 1e3)
    return res


def line(what, pair, res, extra):
    r = {"what": what, "pair": pair}
    for k, v in res.items():
        r[k + "_ms"] = round(float(np.median(v)), 3)
        r[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    r.update(extra)
    return r


def run(B, K, bs, rate, steps, warmup):
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    ch = 2
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    base = np.stack([synth_pcm(s, K * bs, ch, rate, transient=(s % 3 != 1), seed=1) for s in range(16)])
    d_pcm = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 16])).to(dev)
    enc = ulc_amd.BatchEncoder(B, ch, bs, rate, K)
    enc.set_timing(False)
    d_out = torch.empty((B, K, enc.slot), dtype=torch.uint8, device=dev)
    d_bits = torch.empty((B, K), dtype=torch.int32, device=dev)
    s_out, s_bits = torch.empty_like(d_out), torch.empty_like(d_bits)
    d_all = torch.arange(B, dtype=torch.int32, device=dev)
    d_half = torch.arange(0, B, 2, dtype=torch.int32, device=dev)          # every other slot
    d_pcm_half = d_pcm[0::2].contiguous()
    H = int(d_half.numel())
    P = lambda t: t.data_ptr()
    common = {"streams": B, "blocks": K, "block_size": bs, "rate_hz": rate, "steps": 2 * steps, "build": ulc_amd.build_rev()}
    out = []

    enc_forms = {
        "plain": lambda: enc.encode_dev(P(d_pcm), K, P(d_out), P(d_bits), mode=ulc_amd.MODE_VBR, p0=50.0, stream=st.cuda_stream),
        "identity": lambda: enc.encode_subset_dev(P(d_all), B, P(d_pcm), K, P(s_out), P(s_bits), mode=ulc_amd.MODE_VBR, p0=50.0, stream=st.cuda_stream),
        "half": lambda: enc.encode_subset_dev(P(d_half), H, P(d_pcm_half), K, P(s_out), P(s_bits), mode=ulc_amd.MODE_VBR, p0=50.0, stream=st.cuda_stream),
    }
    res = timed(enc_forms, enc.reset, st.synchronize, steps, warmup)
    # the identity call leaves the plain call's sizes behind (same calls since the reset)
    enc.reset(); enc_forms["plain"](); enc.reset(); enc_forms["identity"](); st.synchronize()
    same = bool(torch.equal(d_bits, s_bits))
    state = enc.state_bytes - 16
    est = 4 * state * B / (COPY_TBPS * 1e12) * 1e3         # gather and scatter: a read and a write of every slot's state each
    over = float(np.median(res["identity"]) - np.median(res["plain"]))
    out.append(line("encode", "identity vs plain", {k: res[k] for k in ("plain", "identity")},
                    dict(common, overhead_ms=round(over, 3), copy_estimate_ms=round(est, 3), overhead_over_estimate=round(over / est, 2), sizes_equal=same)))
    out.append(line("encode", f"subset of {H} vs plain of {B}", {k: res[k] for k in ("plain", "half")},
                    dict(common, ratio=round(float(np.median(res["half"]) / np.median(res["plain"])), 4))))
    enc.close()

    # decode: the blocks the encoder just wrote for every stream (slot form)
    slot = int(d_out.shape[2])
    dec = ulc_amd.BatchDecoder(B, ch, bs, K)
    dec.set_timing(False)
    d_in_half = d_out[0::2].contiguous()
    o_pcm = torch.empty((B, K, bs, ch), dtype=torch.float32, device=dev)
    o_bits, t_bits = torch.empty_like(d_bits), torch.empty_like(d_bits)
    dec_forms = {
        "plain": lambda: dec.decode_dev(P(d_out), slot, K, P(o_pcm), P(o_bits), stream=st.cuda_stream),
        "identity": lambda: dec.decode_subset_dev(P(d_all), B, P(d_out), slot, K, P(o_pcm), P(t_bits), stream=st.cuda_stream),
        "half": lambda: dec.decode_subset_dev(P(d_half), H, P(d_in_half), slot, K, P(o_pcm), P(t_bits), stream=st.cuda_stream),
    }
    res = timed(dec_forms, dec.reset, st.synchronize, steps, warmup)
    dec.reset(); dec_forms["plain"](); dec.reset(); dec_forms["identity"](); st.synchronize()
    same = bool(torch.equal(o_bits, t_bits))
    state = dec.state_bytes - 16
    est = 4 * state * B / (COPY_TBPS * 1e12) * 1e3
    over = float(np.median(res["identity"]) - np.median(res["plain"]))
    out.append(line("decode", "identity vs plain", {k: res[k] for k in ("plain", "identity")},
                    dict(common, overhead_ms=round(over, 3), copy_estimate_ms=round(est, 3), overhead_over_estimate=round(over / est, 2), sizes_equal=same)))
    out.append(line("decode", f"subset of {H} vs plain of {B}", {k: res[k] for k in ("plain", "half")},
                    dict(common, ratio=round(float(np.median(res["half"]) / np.median(res["plain"])), 4))))
    dec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per form and round (two rounds, forms alternating)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--block-size", type=int, default=2048)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slots_bench.txt"))
    a = ap.parse_args()
    lines = run(a.streams, a.blocks, a.block_size, a.rate, a.steps, a.warmup)
    with open(a.out, "a") as f:
        for r in lines:
            s = json.dumps(r)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
