"""Device time of ulcx_corpus_splice_dev beside what a caller does without it, at stereo 2048:

    python tools/splice_bench.py [--steps N] [--warmup W] [--clips N] [--out FILE]

(a) rung switch: a two-rung VBR (50 / 20) from_clips_ladder corpus of 4096 clips of 31 blocks becomes 4096 files that switch
    rung every block (31 one-block segments per file);
(b) trim: 64 files of 4096 blocks (joined from the clips of rung 0 by a splice call of their own, checked against the serial
    walk) become 4096 files of 31 blocks at random starts.
Per workload: the call (hipEvents around it on the stream it runs on, --steps timed calls after a warm-up, the forms
alternating in one process); its kernels one by one (torch.profiler's device times over the timed calls; null where the
profiler reports no kernels); ulcx_index_packed_rows_dev on the call's output - the serial walk a caller needs today; a
device-to-device copy of the bytes the call writes, the floor for k_splice_copy; and the whole of today's path in wall time:
download payloads and index, concatenate on the host through the index, upload, ulcx_index_packed_rows_dev, synchronise.
The call's index is compared entry for entry with that walk's, and its payload with the host concatenation, before anything is
timed.  One JSON line per workload with the library's build revision, appended to --out (default profiles/splice_bench.txt).
Not measured here: other geometries, the host forms, corpus.py's path (CropCorpus.splice adds the sizing read and allocations)."""
import argparse
import json
import os
import sys
import time
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
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4), "calls": len(v)}


def kernel_times(fn, calls, torch):
    """Device time per kernel of `calls` calls of fn -> {kernel: {median_us, min_us, max_us}} or None."""
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            name = ev.name
            if "k_splice" in name or "k_dindex_begin" in name:
                short = name.split("(")[0].split("<")[0].replace("void ", "")
                us = float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
                if us > 0:
                    per.setdefault(short, []).append(us)
        if not per:
            return None
        return {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "launches": len(v)} for k, v in sorted(per.items())}
    except Exception as e:                                  # the numbers above do not depend on the profiler
        return {"error": f"{type(e).__name__}: {e}"[:200]}


class Strided:
    """A strided corpus on the device: payload [F][stride], nbytes, index [F][istride][2], blocks."""

    def __init__(self, payload, nbytes, index, blocks):
        self.payload, self.nbytes, self.index, self.blocks = payload, nbytes, index, blocks
        self.F, self.stride, self.istride = payload.shape[0], payload.shape[1], index.shape[1]


def workload(a, emit, torch, dec, what, src, seg_offs, seg, dev):
    """Time one splice of `src` under (seg_offs int32 [nOut + 1], seg int32 [nSeg][3]) and the comparisons."""
    n_out, n_seg = len(seg_offs) - 1, len(seg)
    # sizes from the source index, on the host (as CropCorpus.splice sizes its output on the device)
    offs = src.index[:, :, 0].cpu().numpy().astype(np.int64)
    nbytes = offs[seg[:, 0], seg[:, 1] + seg[:, 2]] - offs[seg[:, 0], seg[:, 1]]
    owner = np.repeat(np.arange(n_out), np.diff(seg_offs))
    per_bytes, per_blocks = np.bincount(owner, nbytes, n_out).astype(np.int64), np.bincount(owner, seg[:, 2], n_out).astype(np.int64)
    stride, istride = (int(per_bytes.max()) + 64 + 15) & ~15, int(per_blocks.max()) + 1
    mk = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
    o_pay, o_nb, o_max, o_idx, o_cnt, o_ss = mk(n_out, stride), mk(n_out, dt=torch.int32), mk(n_out, dt=torch.int32), mk(n_out, istride, 2, dt=torch.int32), \
        mk(n_out, dt=torch.int32), mk(n_seg, dt=torch.int32)
    d_offs, d_seg = torch.from_numpy(seg_offs.astype(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)

    def splice():
        dec.corpus_splice_dev(src.F, src.payload.data_ptr(), src.stride, src.nbytes.data_ptr(), src.index.data_ptr(), src.istride, src.blocks.data_ptr(),
                              n_out, d_offs.data_ptr(), d_seg.data_ptr(), n_seg, o_pay.data_ptr(), stride, o_nb.data_ptr(), o_max.data_ptr(), o_idx.data_ptr(), istride,
                              o_cnt.data_ptr(), o_ss.data_ptr())
    w_idx, w_cnt = mk(n_out, istride, 2, dt=torch.int32), mk(n_out, dt=torch.int32)

    def walk(pay=o_pay, nb=o_nb):
        dec.index_packed_rows_dev(n_out, pay.data_ptr(), stride, nb.data_ptr(), istride - 1, w_idx.data_ptr(), w_cnt.data_ptr())
    total = int(per_bytes.sum())
    flat_src, flat_dst = mk(total), mk(total)

    def floor():
        flat_dst.copy_(flat_src)
    u_pay, u_nb = mk(n_out, stride), mk(n_out, dt=torch.int32)

    def today():
        """download, host concatenation through the index, upload, the serial walk; -> the host payload"""
        h_pay, h_idx = src.payload.cpu().numpy(), src.index[:, :, 0].cpu().numpy()
        out = np.zeros((n_out, stride), np.uint8)
        lens = np.zeros(n_out, np.int32)
        for o in range(n_out):
            parts = [h_pay[f, h_idx[f, k]:h_idx[f, k + c]] for f, k, c in seg[seg_offs[o]:seg_offs[o + 1]]]
            row = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
            out[o, :len(row)] = row
            lens[o] = len(row)
        u_pay.copy_(torch.from_numpy(out)); u_nb.copy_(torch.from_numpy(lens))
        walk(u_pay, u_nb)
        torch.cuda.synchronize()
        return out, lens

    splice(); walk()
    torch.cuda.synchronize()
    same_index = bool(torch.equal(o_idx, w_idx)) and bool(torch.equal(o_cnt, w_cnt)) and np.array_equal(o_cnt.cpu().numpy(), per_blocks)
    h_out, h_lens = today()
    got = o_pay.cpu().numpy()
    mask = np.arange(stride)[None, :] < h_lens[:, None]
    same_bytes = np.array_equal(o_nb.cpu().numpy(), h_lens) and np.array_equal(got[mask], h_out[mask])
    wall = []
    for _ in range(a.today):
        t0 = time.perf_counter()
        today()
        wall.append((time.perf_counter() - t0) * 1e3)
    r = timed({"splice": splice, "index_packed_rows": walk, "d2d_copy": floor}, a.steps, a.warmup, torch)
    line = {"what": what, "source_files": src.F, "output_files": n_out, "segments": n_seg, "blocks": int(per_blocks.sum()), "bytes": total,
            "out_payload_stride": stride, "out_index_stride": istride, "index_equals_serial_walk": same_index, "payload_equals_host_concatenation": bool(same_bytes),
            "splice_call": stats(r["splice"]), "kernels": kernel_times(splice, a.steps, torch), "index_packed_rows_on_output": stats(r["index_packed_rows"]),
            "d2d_copy_of_bytes": stats(r["d2d_copy"]), "today_download_concat_upload_walk_wall": stats(wall),
            "walk_over_splice": round(float(np.median(r["index_packed_rows"]) / np.median(r["splice"])), 2),
            "today_over_splice": round(float(np.median(wall) / np.median(r["splice"])), 1)}
    emit(line)
    assert same_index and same_bytes, "the call's output differs from the serial walk / the host concatenation"
    return Strided(o_pay, o_nb, o_idx, o_cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--today", type=int, default=3, help="timed runs of today's host path (wall time)")
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--only", default="", help="comma list of a,b; default: both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    import corpus
    from ulc_testlib import synth_pcm
    dev = torch.device("cuda:0")
    rev = ulc_amd.build_rev()
    out = open(a.out, "a")

    def emit(d):
        d["build"] = rev
        line = json.dumps(d)
        print(line, flush=True)
        out.write(line + "\n"); out.flush()

    bs, ch, rate, n, nb = 2048, 2, 44100, a.clips, 31
    T = (nb - 2) * bs
    assert ulc_amd.clip_blocks(bs, T) == nb
    base = np.stack([np.ascontiguousarray(synth_pcm(s, T, ch, rate, transient=(s % 3 != 1), seed=1).T) for s in range(16)])
    wave = torch.from_numpy(base).to(dev)[torch.from_numpy(np.arange(n) % 16).to(dev)].contiguous()          # [n][2][T]
    enc = ulc_amd.BatchEncoder(n, ch, bs, rate, 11)
    dec = ulc_amd.BatchDecoder(1, ch, bs, 1)                 # geometry and tables are all the splice and index calls read of it
    cor = corpus.CropCorpus.from_clips_ladder(enc, dec, wave, rates=((ulc_amd.MODE_VBR, 50.0), (ulc_amd.MODE_VBR, 20.0)), payload_stride=48 * 1024)
    torch.cuda.synchronize()
    del wave
    assert int(cor.d_index_blocks.min().item()) == nb, "a clip's file does not hold all its blocks"
    ladder = Strided(cor.d_payload, cor.d_payload_bytes, cor.d_index, cor.d_index_blocks)
    only = set(a.only.split(",")) if a.only else set("ab")
    rng = np.random.default_rng(7)
    if "a" in only:
        k = np.tile(np.arange(nb), n)
        clip = np.repeat(np.arange(n), nb)
        seg = np.stack([((k + clip) & 1) * n + clip, k, np.ones_like(k)], axis=1)      # clip c starts on rung c & 1 and switches every block
        workload(a, emit, torch, dec, f"(a) rung switch: {n} clips x {nb} blocks under VBR 50 / VBR 20 -> {n} files that switch rung every block", ladder,
                 np.arange(0, n * nb + 1, nb), seg, dev)
    if "b" in only:
        # 64 files of 4096 blocks: the clips of rung 0, whole, one behind the other (a splice call of its own, not timed)
        F, L = 64, 4096
        per = -(-L // nb)
        files = rng.integers(0, n, (F, per))
        counts = np.full((F, per), nb); counts[:, -1] = L - nb * (per - 1)
        seg = np.stack([files.reshape(-1), np.zeros(F * per, np.int64), counts.reshape(-1)], axis=1)
        long_files = _join(torch, dec, ladder, np.arange(0, F * per + 1, per), seg, dev)
        assert int(long_files.blocks.min().item()) == L
        starts = rng.integers(0, L - nb + 1, n)
        seg = np.stack([rng.integers(0, F, n), starts, np.full(n, nb)], axis=1)
        workload(a, emit, torch, dec, f"(b) trim: {F} files x {L} blocks (VBR 50) -> {n} files of {nb} blocks at random starts", long_files, np.arange(n + 1), seg, dev)
    out.close()
    enc.close(); dec.close()


def _join(torch, dec, src, seg_offs, seg, dev):
    """The input of (b): one splice call, its index checked against the serial walk of its payload."""
    n_out, n_seg = len(seg_offs) - 1, len(seg)
    offs = src.index[:, :, 0].cpu().numpy().astype(np.int64)
    nbytes = offs[seg[:, 0], seg[:, 1] + seg[:, 2]] - offs[seg[:, 0], seg[:, 1]]
    owner = np.repeat(np.arange(n_out), np.diff(seg_offs))
    stride = (int(np.bincount(owner, nbytes, n_out).max()) + 64 + 15) & ~15
    istride = int(np.bincount(owner, seg[:, 2], n_out).max()) + 1
    mk = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
    o = Strided(mk(n_out, stride), mk(n_out, dt=torch.int32), mk(n_out, istride, 2, dt=torch.int32), mk(n_out, dt=torch.int32))
    ss, w_idx, w_cnt = mk(n_seg, dt=torch.int32), mk(n_out, istride, 2, dt=torch.int32), mk(n_out, dt=torch.int32)
    d_offs, d_seg = torch.from_numpy(seg_offs.astype(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(seg, np.int32)).to(dev)
    dec.corpus_splice_dev(src.F, src.payload.data_ptr(), src.stride, src.nbytes.data_ptr(), src.index.data_ptr(), src.istride, src.blocks.data_ptr(),
                          n_out, d_offs.data_ptr(), d_seg.data_ptr(), n_seg, o.payload.data_ptr(), stride, o.nbytes.data_ptr(), 0, o.index.data_ptr(), istride,
                          o.blocks.data_ptr(), ss.data_ptr())
    dec.index_packed_rows_dev(n_out, o.payload.data_ptr(), stride, o.nbytes.data_ptr(), istride - 1, w_idx.data_ptr(), w_cnt.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.equal(o.index, w_idx)) and bool(torch.equal(o.blocks, w_cnt)), "the joined files' index differs from the serial walk"
    return o


if __name__ == "__main__":
    main()
