"""Wall clock of the clips call (ulcx_encode_clips_dev) beside what a caller does without it, and of ulcx_corpus_ragged_dev beside
the host's re-lay: synchronised calls on device buffers, 20 timed calls per form after a warm-up, the forms alternating in one
process (tools/sample_crops_bench.py's pattern).

    python tools/clips_bench.py [--steps N] [--warmup W] [--rows N] [--out FILE]

4096 stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1] samples, held as one torch batch [4096][2][61441];
VBR 50; an encoder of 4096 streams with maxBlocksPerCall = 11 (a clip has up to 33 blocks: three chunks).  The forms:
  clips        (a) the clips call: payloads, byte counts, index and block counts in one asynchronous call
  today        (b) the same corpus with the calls the library had before: torch mask + pad, transpose and contiguous();
               reset_streams; per chunk a contiguous() of the chunk, ulcx_encode_dev_rates, the chunk's slots and masked sizes
               copied into whole-clip buffers; then ONE ulcx_pack_streams_dev and ONE index_begin / index_slots over all 33
               blocks.  (Cheaper than a pack call per chunk plus a concatenation of ragged rows, which torch has no pass for.)
  ragged       (c) ulcx_corpus_ragged_dev on (a)'s corpus: the sizing call, the 16-byte read of the totals, the allocation, the call
  ragged_host  (c') corpus.py::_layout_ragged on host copies of the same files plus the upload of its five arrays
Before anything is timed (a)'s outputs are compared byte for byte with (b)'s, and (c)'s with (c')'s.
One JSON line with the library's build revision, appended to --out (default profiles/clips_bench.txt)."""
import argparse
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crops_bench import timed, stats, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_bench.txt"))
    a = ap.parse_args()
    import torch
    import ulc_amd
    import corpus
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
    d_nbk = torch.from_numpy(h_nb.astype(np.int32)).to(dev)
    d_rate = torch.tensor([[-50.0, 0.0]] * n, dtype=torch.float32, device=dev)

    enc = ulc_amd.BatchEncoder(n, ch, bs, rate, maxk)
    dec = ulc_amd.BatchDecoder(1, ch, bs, 1)
    stride, istride = 96 * 1024, nb_max + 1
    mk = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)
    A = dict(pay=mk(n, stride), nbytes=mk(n, dt=torch.int32), maxb=mk(n, dt=torch.int32), idx=mk(n, istride, 2, dt=torch.int32), cnt=mk(n, dt=torch.int32))
    Bf = dict(pay=mk(n, stride), nbytes=mk(n, dt=torch.int32), maxb=mk(n, dt=torch.int32), idx=mk(n, istride, 2, dt=torch.int32), cnt=mk(n, dt=torch.int32))
    slots_all = mk(n, nb_max, enc.slot)
    bits_all = mk(n, nb_max, dt=torch.int32)
    c_out = mk(n, maxk, enc.slot)
    c_bits = mk(n, maxk, dt=torch.int32)
    all_slots = torch.arange(n, dtype=torch.int32, device=dev)
    t_idx = torch.arange(T, device=dev)
    k_idx = torch.arange(nb_max, device=dev)

    def clips():
        enc.encode_clips_dev(dec, n, wave.data_ptr(), d_len.data_ptr(), T, A["pay"].data_ptr(), stride, A["nbytes"].data_ptr(), A["idx"].data_ptr(), istride,
                             A["cnt"].data_ptr(), d_max_block=A["maxb"].data_ptr(), mode=ulc_amd.MODE_VBR, p0=50.0)

    def today():
        x = torch.nn.functional.pad(wave * (t_idx[None, None, :] < d_len[:, None, None]), (0, nb_max * bs - T))        # mask + pad to whole blocks
        x = x.transpose(1, 2).contiguous()                                                                              # [n][33 * bs][2]
        enc.reset_streams_dev(all_slots.data_ptr(), n)
        for k0 in range(0, nb_max, maxk):
            K = min(maxk, nb_max - k0)
            chunk = x[:, k0 * bs:(k0 + K) * bs].contiguous()
            enc.encode_dev_rates(d_rate.data_ptr(), chunk.data_ptr(), K, c_out.data_ptr(), c_bits.data_ptr())
            slots_all[:, k0:k0 + K] = c_out.view(-1)[:n * K * enc.slot].view(n, K, enc.slot)
            bits_all[:, k0:k0 + K] = c_bits.view(-1)[:n * K].view(n, K)
        bits_all.mul_(k_idx[None, :] < d_nbk[:, None])                                                                  # the tool's mask behind every row's end
        rc = ulc_amd.lib().ulcx_pack_streams_dev(0, n, nb_max, enc.slot, slots_all.data_ptr(), bits_all.data_ptr(), Bf["pay"].data_ptr(), stride,
                                                 Bf["nbytes"].data_ptr(), Bf["maxb"].data_ptr(), None)
        assert rc == 0
        dec.index_begin_dev(n, Bf["idx"].data_ptr(), istride, Bf["cnt"].data_ptr())
        dec.index_slots_dev(n, slots_all.data_ptr(), enc.slot, bits_all.data_ptr(), nb_max, Bf["idx"].data_ptr(), istride, Bf["cnt"].data_ptr())

    clips(); today(); sync()
    cnt = A["cnt"].cpu().numpy()
    assert np.array_equal(cnt, h_nb), "a row was truncated: the stride is too small for this input"
    valid = torch.arange(stride, device=dev)[None, :] < A["nbytes"][:, None]
    same = bool(torch.equal(A["nbytes"], Bf["nbytes"]) and torch.equal(A["maxb"], Bf["maxb"]) and torch.equal(A["cnt"], Bf["cnt"]) and torch.equal(A["idx"], Bf["idx"])
                and torch.equal(A["pay"] * valid, Bf["pay"] * valid))

    # (c) / (c'): the corpus of (a) into the ragged layout
    R = {}
    none = mk(16)
    poffs, ioffs, oblocks, need = mk(n + 1, dt=torch.int64), mk(n + 1, dt=torch.int64), mk(n, dt=torch.int32), mk(2, dt=torch.int64)
    src = (n, A["pay"].data_ptr(), stride, A["nbytes"].data_ptr(), A["idx"].data_ptr(), istride, A["cnt"].data_ptr())

    def ragged():
        ulc_amd.corpus_ragged_dev(*src, none.data_ptr(), 0, poffs.data_ptr(), none.data_ptr(), 0, ioffs.data_ptr(), oblocks.data_ptr(), need.data_ptr())
        nby, nen = (int(v) for v in need.cpu())
        R["pay"] = torch.empty(nby + corpus.PAYLOAD_PAD, dtype=torch.uint8, device=dev)
        R["idx"] = torch.empty((nen, 2), dtype=torch.int32, device=dev)
        ulc_amd.corpus_ragged_dev(*src, R["pay"].data_ptr(), nby, poffs.data_ptr(), R["idx"].data_ptr(), nen, ioffs.data_ptr(), oblocks.data_ptr(), need.data_ptr())
        R["need"] = (nby, nen)

    h_pay, h_nby, h_idx = A["pay"].cpu().numpy(), A["nbytes"].cpu().numpy(), A["idx"].cpu().numpy()
    host = corpus.CropCorpus(ch, bs, layout="ragged")
    for f in range(n):
        host._payloads.append(h_pay[f, :h_nby[f]].tobytes())
        host._index.append(np.ascontiguousarray(h_idx[f, :cnt[f] + 1]).view(ulc_amd.INDEX_DTYPE).reshape(-1))
        host._blocks.append(int(cnt[f]))
    H = {}

    def ragged_host():
        lay = host._layout_ragged()
        H["pay"] = torch.from_numpy(lay["payload"]).to(dev)
        H["poffs"] = torch.from_numpy(lay["payload_offs"]).to(dev)
        H["idx"] = torch.from_numpy(lay["index"].view(np.int32).reshape(-1, 2)).to(dev)
        H["ioffs"] = torch.from_numpy(lay["index_offs"]).to(dev)
        H["blocks"] = torch.from_numpy(lay["index_blocks"]).to(dev)

    ragged(); ragged_host(); sync()
    nby = R["need"][0]
    same_ragged = bool(torch.equal(poffs, H["poffs"]) and torch.equal(ioffs, H["ioffs"]) and torch.equal(oblocks, H["blocks"]) and torch.equal(R["idx"], H["idx"])
                       and torch.equal(R["pay"][:nby], H["pay"][:nby]))

    r = timed({"clips": clips, "today": today, "ragged": ragged, "ragged_host": ragged_host}, a.steps, a.warmup, sync)
    s = {k: stats(v) for k, v in r.items()}
    ratio = lambda x, y: round(s[x]["median_ms"] / s[y]["median_ms"], 4)
    blocks = int(h_nb.sum())
    line = {"what": f"{n} stereo clips at BlockSize 2048, lengths uniform in [1, 30 * 2048 + 1], VBR 50, maxBlocksPerCall {maxk}: (a) the clips call, (b) the "
                    "same corpus with torch pad / transpose / contiguous, reset_streams, chunked encode_dev_rates, the sizes' mask, one pack_streams and one "
                    "index_begin / index_slots over all blocks; (c) ulcx_corpus_ragged_dev with its sizing call, (c') _layout_ragged on the host + upload "
                    "(wall clock of synchronised calls)",
            "clips": s["clips"], "today": s["today"], "clips_over_today": ratio("clips", "today"),
            "ragged": s["ragged"], "ragged_host": s["ragged_host"], "ragged_over_host": ratio("ragged", "ragged_host"),
            "outputs_equal": same, "ragged_outputs_equal": same_ragged, "blocks_kept": blocks, "blocks_encoded": n * nb_max,
            "payload_bytes": int(h_nby.astype(np.int64).sum()), "input_bytes": nbytes(wave), "staging_bytes_moved": 2 * n * nb_max * bs * ch * 4,
            "ulcx_build_rev": rev}
    enc.close(); dec.close()
    text = json.dumps(line)
    print(text, flush=True)
    with open(a.out, "a") as out:
        out.write(text + "\n")


if __name__ == "__main__":
    main()
