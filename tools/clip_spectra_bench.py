"""Clip spectra (ulcx_analyse_clips_dev, ulcx_encode_clips_spectra_dev) at tools/clips_bench.py's shape: 4096 stereo clips at
BlockSize 2048 held as one torch batch [4096][2][61441], lengths uniform in [1, 30 * 2048 + 1] samples, VBR 50, an encoder of 4096
streams with maxBlocksPerCall = 11 (a clip has up to 33 blocks: three chunks); planes 33 blocks deep.

    python tools/clip_spectra_bench.py [--steps N] [--warmup W] [--rows N] [--only a,b,...] [--out FILE]
    python tools/clip_spectra_bench.py --trace [--steps N]          # under rocprofv3 --kernel-trace, in a run of its own
    python tools/clip_spectra_bench.py --summarise DIR [--out FILE] # the trace's k_clip_spec and copy durations

Wall clock of synchronised calls, the forms alternating call by call in one process (tools/crops_bench.py's pattern):
  clips          ulcx_encode_clips_dev: the plain clips call (the only form a library without the tap has: --only clips)
  clips_spectra  ulcx_encode_clips_spectra_dev, flags 0: the same corpus and the clean spectra
  analyse_clips  ulcx_analyse_clips_dev, flags 0
  today          the route to the same coefficients without these calls (timed --today-steps times): torch mask + pad + transpose,
                 reset_streams, per chunk ulcx_encode_dev and ulcx_encoder_debug_fetch of its coefficients - the tap refuses after
                 an analysis call, so the chunk is encoded - and a numpy transpose into [n][nChan][blocks][BlockSize] on the host
Before anything is timed the encode form's corpus is compared with the plain call's, the two forms' planes with each other, and
today's coefficients with them on the live blocks.
--trace runs the encode form with flags 0 and with ULCX_SPECTRA_LR and, per chunk, a hipMemcpyDtoDAsync of the bytes one launch
of k_clip_spec writes (read N, write N); --summarise reads the kernel trace (and the memory-copy trace, if the copy went there).
One JSON line per run with the library's build revision, appended to --out (default profiles/clip_spectra_bench.txt)."""
import argparse
import csv
import ctypes
import glob
import json
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crops_bench import timed, stats, nbytes


def summarise(directory, out, skip):
    """Durations (us) of the k_clip_spec launches and of the copies of the trace under `directory`, each kind without its first
    `skip` (the warm-up calls' three chunks): median, min .. max, count."""
    groups = {}
    dur = lambda r: (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"]
            key = ("k_clip_spec<LR>" if re.search(r"k_clip_spec<\s*true|k_clip_specILb1", name) else
                   "k_clip_spec<0>" if "k_clip_spec" in name else "copy kernel " + name[:60] if re.search("copy", name, re.I) else None)
            if key:
                groups.setdefault(key, []).append(dur(r))
    for path in glob.glob(os.path.join(directory, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "DEVICE_TO_DEVICE" in r.get("Direction", "").upper():
                groups.setdefault("memory copy, device to device", []).append(dur(r))
    groups = {k: [d for _, d in sorted(v)[skip:]] for k, v in groups.items() if len(v) > skip}
    line = {"what": "rocprofv3 trace of tools/clip_spectra_bench.py --trace: durations in microseconds per launch / copy",
            "skipped_per_kind": skip, "trace": {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "count": len(v)} for k, v in sorted(groups.items())}}
    text = json.dumps(line)
    print(text, flush=True)
    with open(out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--today-steps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--only", default="", help="comma list of clips,clips_spectra,analyse_clips,today; default: all")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_spectra_bench.txt"))
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.out, 3 * a.warmup)
    import torch
    import ulc_amd
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    sync = torch.cuda.synchronize
    only = set(a.only.split(",")) if a.only else {"clips", "clips_spectra", "analyse_clips", "today"}

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
    corpus_bufs = lambda: dict(pay=mk(n, stride), nbytes=mk(n, dt=torch.int32), maxb=mk(n, dt=torch.int32), idx=mk(n, istride, 2, dt=torch.int32), cnt=mk(n, dt=torch.int32))
    planes = lambda: dict(coef=mk(n, ch, nb_max, bs, dt=torch.float32), wc=mk(n, nb_max, dt=torch.int32), cplx=mk(n, nb_max, dt=torch.float32))
    A, S = corpus_bufs(), corpus_bufs()
    corpus_args = lambda B: (dec, n, wave.data_ptr(), d_len.data_ptr(), T, B["pay"].data_ptr(), stride, B["nbytes"].data_ptr(), B["idx"].data_ptr(), istride, B["cnt"].data_ptr())

    def clips():
        enc.encode_clips_dev(*corpus_args(A), d_max_block=A["maxb"].data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)

    if only == {"clips"}:                                   # a library without the tap: the plain call alone
        r = timed({"clips": clips}, a.steps, a.warmup, sync)
        line = {"what": f"{n} stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1], VBR 50, maxBlocksPerCall {maxk}: the plain clips call alone",
                "clips": stats(r["clips"]), "ulcx_build_rev": rev}
        return finish(line, a.out, enc, dec)

    P, Q = planes(), planes()

    def clips_spectra(flags=0):
        enc.encode_clips_spectra_dev(*corpus_args(S), nb_max, P["coef"].data_ptr(), P["wc"].data_ptr(), P["cplx"].data_ptr(), flags=flags,
                                     d_max_block=S["maxb"].data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)

    def analyse_clips():
        enc.analyse_clips_dev(n, wave.data_ptr(), d_len.data_ptr(), T, nb_max, Q["coef"].data_ptr(), Q["wc"].data_ptr(), Q["cplx"].data_ptr())

    launch_bytes = n * maxk * ch * bs * 4                   # what one launch of k_clip_spec writes (every chunk has 11 blocks)
    if a.trace:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        src, dst = mk(launch_bytes), mk(launch_bytes)
        for i in range(a.warmup + a.steps):
            clips_spectra(0); sync()
            clips_spectra(ulc_amd.SPECTRA_LR); sync()
            for _ in range(nb_max // maxk):
                assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), launch_bytes, None) == 0
                sync()
        print(json.dumps({"traced": a.warmup + a.steps, "launch_bytes": launch_bytes, "ulcx_build_rev": rev}), flush=True)
        enc.close(); dec.close()
        return

    t_idx = torch.arange(T, device=dev)
    all_slots = torch.arange(n, dtype=torch.int32, device=dev)
    c_out, c_bits = mk(n, maxk, enc.slot), mk(n, maxk, dt=torch.int32)
    H = {}

    def today():
        x = torch.nn.functional.pad(wave * (t_idx[None, None, :] < d_len[:, None, None]), (0, nb_max * bs - T))        # mask + pad to whole blocks
        x = x.transpose(1, 2).contiguous()                                                                              # [n][33 * bs][2]
        enc.reset_streams_dev(all_slots.data_ptr(), n)
        out = np.empty((n, ch, nb_max, bs), np.float32)
        for k0 in range(0, nb_max, maxk):
            K = min(maxk, nb_max - k0)
            chunk = x[:, k0 * bs:(k0 + K) * bs].contiguous()
            enc.encode_dev(chunk.data_ptr(), K, c_out.data_ptr(), c_bits.data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)
            coef = enc.debug_fetch(K=K, parts=("coef",))["coef"]                                                         # [n][K][ch * bs] on the host
            out[:, :, k0:k0 + K] = coef.reshape(n, K, ch, bs).transpose(0, 2, 1, 3)
        H["coef"] = out

    clips(); clips_spectra(); analyse_clips(); sync()
    valid = torch.arange(stride, device=dev)[None, :] < A["nbytes"][:, None]
    same_corpus = bool(torch.equal(A["nbytes"], S["nbytes"]) and torch.equal(A["maxb"], S["maxb"]) and torch.equal(A["cnt"], S["cnt"]) and torch.equal(A["idx"], S["idx"])
                       and torch.equal(A["pay"] * valid, S["pay"] * valid))
    assert np.array_equal(A["cnt"].cpu().numpy(), h_nb), "a row was truncated: the stride is too small for this input"
    same_planes = bool(torch.equal(P["coef"].view(torch.int32), Q["coef"].view(torch.int32)) and torch.equal(P["wc"], Q["wc"])
                       and torch.equal(P["cplx"].view(torch.int32), Q["cplx"].view(torch.int32)))
    same_today = None
    if "today" in only:
        today(); sync()
        live = (np.arange(nb_max)[None, :] < h_nb[:, None])[:, None, :, None]
        same_today = bool(np.array_equal(np.where(live, H["coef"], np.float32(0)).view(np.uint32), P["coef"].cpu().numpy().view(np.uint32)))

    fns = {k: f for k, f in (("clips", clips), ("clips_spectra", clips_spectra), ("analyse_clips", analyse_clips)) if k in only}
    r = timed(fns, a.steps, a.warmup, sync)
    if "today" in only:
        r.update(timed({"today": today}, a.today_steps, 1, sync))
    s = {k: stats(v) for k, v in r.items()}
    ratio = lambda x, y: round(s[x]["median_ms"] / s[y]["median_ms"], 4) if x in s and y in s else None
    line = {"what": f"{n} stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1], VBR 50, maxBlocksPerCall {maxk}, planes {nb_max} blocks deep: the plain "
                    "clips call, the encode form with the tap, the analysis form, and today's route (torch pad / transpose, reset_streams, per chunk ulcx_encode_dev + "
                    "ulcx_encoder_debug_fetch of the coefficients, numpy transpose on the host); wall clock of synchronised calls",
            **s, "spectra_over_clips": ratio("clips_spectra", "clips"), "analyse_over_spectra": ratio("analyse_clips", "clips_spectra"),
            "analyse_over_today": ratio("analyse_clips", "today"), "corpus_equal": same_corpus, "planes_equal": same_planes, "today_equal_on_live_blocks": same_today,
            "blocks_live": int(h_nb.sum()), "blocks_in_planes": n * nb_max, "plane_bytes": nbytes(P["coef"]), "launch_bytes": launch_bytes, "ulcx_build_rev": rev}
    finish(line, a.out, enc, dec)


def finish(line, out, enc, dec):
    enc.close(); dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
