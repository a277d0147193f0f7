"""Wall clock of the clips ladder call (ulcx_encode_clips_ladder_dev) beside what it replaces: synchronised calls on device
buffers, 20 timed calls per form after a warm-up, the forms alternating in one process (tools/clips_bench.py's pattern and shape).

    python tools/clips_ladder_bench.py [--steps N] [--warmup W] [--rows N] [--only plain] [--out FILE]

4096 stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1] samples, held as one torch batch [4096][2][61441]; an
encoder of 4096 streams with maxBlocksPerCall = 11 (a clip has up to 33 blocks: three chunks).  The forms:
  ladder2 / ladder4   (a) ONE ladder call with 2 / 4 scalar VBR rungs (quality 30, 70 / 30, 50, 70, 90)
  plain2 / plain4         the same files by 2 / 4 plain clips calls, each into its own part of one corpus
  auto                (b) ONE ladder call with one ULCX_RUNG_AUTO rung at 64 kbps
  auto_today              ulcx_analyse_clips_dev (its coefficient planes included: the call has no form without them), the
                          download of the [n][33] complexities, the rows' ordered binary64 sums and averages on the host, the
                          upload of the table, ulcx_encode_clips_dev with it
  plain               (c) one plain clips call, VBR 50 - `--only plain` times nothing else, for a run against another build of
                          the library (ULC_AMD_LIB).  In a full run the call is also timed alone on the fresh object
                          (plain_fresh) and alone behind everything, the staging grown to four rungs (plain_grown)
Before anything is timed the ladder's files are compared byte for byte with the plain calls', and auto's with auto_today's.
One JSON line with the library's build revision, appended to --out (default profiles/clips_ladder_bench.txt)."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crops_bench import timed, stats

QUALITY = (30.0, 70.0, 50.0, 90.0)                          # two rungs: the first two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--only", default="", help="plain: the plain clips call alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_ladder_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize

    bs, ch, rate, n, maxk = 2048, 2, 44100, a.rows, 11
    T = 30 * bs + 1
    nb_max = ulc_amd.clip_blocks(bs, T)
    assert nb_max == 33
    rng = np.random.default_rng(5)
    base = np.stack([np.ascontiguousarray(synth_pcm(s, T, ch, rate, transient=(s % 3 != 1), seed=1).T) for s in range(16)])
    wave = torch.from_numpy(base).to(dev)[torch.from_numpy(np.arange(n) % 16).to(dev)].contiguous()          # [n][2][T]
    h_len = rng.integers(1, T + 1, n).astype(np.int32)
    d_len = torch.from_numpy(h_len).to(dev)
    h_nb = (h_len.astype(np.int64) + bs - 1) // bs + 2

    enc = ulc_amd.BatchEncoder(n, ch, bs, rate, maxk)
    dec = ulc_amd.BatchDecoder(1, ch, bs, 1)
    stride, istride = 96 * 1024, nb_max + 1
    mk = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
    corpus_of = lambda files: dict(pay=mk(files, stride), nbytes=mk(files, dt=torch.int32), maxb=mk(files, dt=torch.int32), idx=mk(files, istride, 2, dt=torch.int32),
                                   cnt=mk(files, dt=torch.int32))

    def plain_call(c, f0, mode, p0, d_rates=0):
        """a plain clips call into files [f0, f0 + n) of corpus c"""
        enc.encode_clips_dev(dec, n, wave.data_ptr(), d_len.data_ptr(), T, c["pay"][f0:].data_ptr(), stride, c["nbytes"][f0:].data_ptr(), c["idx"][f0:].data_ptr(), istride,
                             c["cnt"][f0:].data_ptr(), d_max_block=c["maxb"][f0:].data_ptr(), mode=mode, p0=p0, d_rates=d_rates)

    def ladder_call(c, rungs, d_avg=0):
        enc.encode_clips_ladder_dev(dec, n, rungs, wave.data_ptr(), d_len.data_ptr(), T, c["pay"].data_ptr(), stride, c["nbytes"].data_ptr(), c["idx"].data_ptr(), istride,
                                    c["cnt"].data_ptr(), d_max_block=c["maxb"].data_ptr(), d_avg=d_avg)

    def same(x, y):
        valid = torch.arange(stride, device=dev)[None, :] < x["nbytes"][:, None]
        return bool(torch.equal(x["nbytes"], y["nbytes"]) and torch.equal(x["maxb"], y["maxb"]) and torch.equal(x["cnt"], y["cnt"]) and torch.equal(x["idx"], y["idx"])
                    and torch.equal(x["pay"] * valid, y["pay"] * valid))

    P1 = corpus_of(n)
    forms = {"plain": lambda: plain_call(P1, 0, ulc_amd.MODE_VBR, 50.0)}
    line = {"what": f"{n} stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1], maxBlocksPerCall {maxk}: the plain clips call at VBR 50"}
    fresh = None
    if a.only != "plain":
        # the plain call alone on the fresh object, one rung of staging: against `plain_grown` behind the ladder forms below
        fresh = stats(timed({"plain": forms["plain"]}, a.steps, a.warmup, sync)["plain"])
        L, P = corpus_of(4 * n), corpus_of(4 * n)
        for R in (2, 4):
            forms[f"ladder{R}"] = lambda R=R: ladder_call(L, [(ulc_amd.MODE_VBR, q) for q in QUALITY[:R]])
            forms[f"plain{R}"] = lambda R=R: [plain_call(P, r * n, ulc_amd.MODE_VBR, QUALITY[r]) for r in range(R)]
        # (b) AUTO 64 kbps against the host detour
        LA, PA = corpus_of(n), corpus_of(n)
        d_avg = mk(n, dt=torch.float32)
        coef = torch.empty((n, ch, nb_max, bs), dtype=torch.float32, device=dev)
        d_cplx = mk(n, nb_max, dt=torch.float32)
        d_table = mk(n, 2, dt=torch.float32)
        H = {}

        def auto_today():
            enc.analyse_clips_dev(n, wave.data_ptr(), d_len.data_ptr(), T, nb_max, coef.data_ptr(), d_cplx=d_cplx.data_ptr())
            cplx = d_cplx.cpu().numpy()                     # (synchronises)
            s = np.zeros(n, np.float64)
            for k in range(nb_max):                         # block order; blocks behind a row's end are +0 in the plane
                s += cplx[:, k]
            table = np.stack([np.full(n, 64.0, np.float32), (s / h_nb).astype(np.float32)], axis=1)
            H["avg"] = table[:, 1]
            d_table.copy_(torch.from_numpy(table))
            plain_call(PA, 0, 0, 0.0, d_rates=d_table.data_ptr())
        forms["auto"] = lambda: ladder_call(LA, [("auto", 64.0)], d_avg=d_avg.data_ptr())
        forms["auto_today"] = auto_today
        line["what"] += ("; (a) one ladder call with 2 / 4 VBR rungs against 2 / 4 plain calls; (b) one AUTO 64 kbps rung against analyse_clips_dev + download + host "
                         "sums + upload + the clips call with the table (wall clock of synchronised calls)")

    for fn in forms.values():
        fn()
    sync()
    assert np.array_equal(P1["cnt"].cpu().numpy(), h_nb), "a row was truncated: the stride is too small for this input"
    if a.only != "plain":
        assert np.array_equal(L["cnt"].cpu().numpy(), np.tile(h_nb, 4)), "a file was truncated: the stride is too small for this input"
        line["ladder_outputs_equal"] = same(L, P)           # (both hold the four-rung forms' files: they ran last)
        line["auto_outputs_equal"] = same(LA, PA) and d_avg.cpu().numpy().tobytes() == H["avg"].tobytes()
        line["payload_bytes_4_rungs"] = int(L["nbytes"].sum().item())

    r = timed(forms, a.steps, a.warmup, sync)
    s = {k: stats(v) for k, v in r.items()}
    line.update(s)
    if fresh is not None:
        # the same call alone again, the staging grown to four rungs: `plain` above ran between the other forms
        line["plain_fresh"], line["plain_grown"] = fresh, stats(timed({"plain": forms["plain"]}, a.steps, a.warmup, sync)["plain"])
    spread = lambda k: s[k]["max_ms"] - s[k]["min_ms"]
    if a.only != "plain":
        for R in (2, 4):
            line[f"ladder{R}_over_plain{R}"] = round(s[f"ladder{R}"]["median_ms"] / s[f"plain{R}"]["median_ms"], 4)
            # the bar: the ladder lies below the plain calls' sum by more than the two spreads together
            line[f"ladder{R}_gain_ms"] = round(s[f"plain{R}"]["median_ms"] - s[f"ladder{R}"]["median_ms"], 4)
            line[f"ladder{R}_spreads_ms"] = round(spread(f"ladder{R}") + spread(f"plain{R}"), 4)
        line["auto_over_today"] = round(s["auto"]["median_ms"] / s["auto_today"]["median_ms"], 4)
        line["ms_per_extra_rung"] = round((s["ladder4"]["median_ms"] - s["ladder2"]["median_ms"]) / 2, 4)
    line["blocks_kept_per_rung"] = int(h_nb.sum())
    line["ulcx_build_rev"] = rev
    enc.close(); dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
