"""The one model of a packed file and of a corpus of such files behind every decoder-side test family (crops, ragged crops,
sample crops, spectra, distortion, splice, damaged payloads, synthesis from spectra).  It answers two questions from the oracle
alone: what do the buffers hold - payloads, byte offsets, index rows, both layouts of include/ulc_amd.h section 3 - and what
must a row give.  A family's testlib adds its row tables and its referee and nothing of the layout.
CPU only: numpy and the oracle; nothing here imports the library under test (to_device() alone imports torch)."""
import functools
import numpy as np
from ulc_testlib import oracle_decode_stream_coefs, wc_of
from seek_testlib import SEED0, ORACLE_BLOCKS, ORACLE_CASES, SYNTH_SEED, SYNTH_BLOCKS, SYNTH_CASES, geometries, oracle_stream, synth_stream, oracle_seeds, oracle_pcm, expected_range

INDEX_DTYPE = np.dtype([("ByteOffs", np.int32), ("RngState", np.uint32)])     # ulcx_index_entry; tests/test_corpus_model.py holds it to ulc_amd's
PAD = 64                                                   # bytes behind the longest (strided) or the last (ragged) payload (corpus.PAYLOAD_PAD)


def to_lr(coef):
    """coef [..., C, N, bs] -> the pairs (0,1), (2,3), ... as m + s, m - s in float32; a trailing single channel unchanged."""
    out = np.array(coef, np.float32, copy=True)
    ch = out.shape[-3]
    for c in range(0, ch - 1, 2):
        m, s = coef[..., c, :, :].astype(np.float32), coef[..., c + 1, :, :].astype(np.float32)
        out[..., c, :, :] = m + s
        out[..., c + 1, :, :] = m - s
    return out


class File:
    """One packed file.  blocks: slot-form rows [K][slot]; bits: the sizes its writer reports (an encoder's, whole bytes, or a
    decoder's, exact: both round up to the same bytes).  payload uint8 [nbytes], nb / offs int64 [K] / [K + 1], wc [K] from every
    block's first byte; the oracle's answers - generator states, sequential decode, coefficients - are computed when first read."""

    def __init__(self, name, bs, ch, blocks, bits):
        self.name, self.bs, self.ch, self.K = name, bs, ch, len(bits)
        self.blocks, self.bits = np.ascontiguousarray(blocks), np.asarray(bits, np.int32)
        self.nb = (self.bits.astype(np.int64) + 7) // 8
        self.offs = np.concatenate([[0], np.cumsum(self.nb)]).astype(np.int64)
        self.payload = np.concatenate([self.blocks[k, :self.nb[k]] for k in range(self.K)]).astype(np.uint8)
        self.wc = wc_of(self.blocks)

    @functools.cached_property
    def seeds(self):
        """uint32 [K + 1]: the generator's state in front of every block and behind the last."""
        return oracle_seeds(self.blocks, self.ch, self.bs)

    @functools.cached_property
    def _decode(self):
        return oracle_pcm(self.blocks, self.ch, self.bs)

    @property
    def pcm(self):
        """[K][bs][ch]: the oracle's sequential decode from block 0."""
        return self._decode[0]

    @property
    def obits(self):
        """int32 [K]: the sizes the oracle's decoder reports, exact."""
        return self._decode[1]

    @functools.cached_property
    def coef(self):
        """[K][C][bs]: the dequantised coefficients the oracle's decoder holds for every block."""
        rc, _, obits, coefs = oracle_decode_stream_coefs(self.blocks, self.ch, self.bs)
        # (an encoder's size is its block rounded up to a byte; the decoder's, which the calls report, is exact)
        assert rc == 0 and np.array_equal((obits + 7) // 8, self.nb) and np.array_equal(obits, self.obits), self.name
        return coefs.reshape(self.K, self.ch, self.bs)

    def row(self, cap=None, blocks=None):
        """The file's index row of `cap` entries (default: blocks + 1) as the index calls fill one: the first `blocks` blocks,
        {-1, 0} behind the closing entry."""
        n = self.K if blocks is None else blocks
        cap = n + 1 if cap is None else cap
        r = np.zeros(cap, INDEX_DTYPE)
        r["ByteOffs"] = -1
        r["ByteOffs"][:n + 1] = self.offs[:n + 1]
        r["RngState"][:n + 1] = self.seeds[:n + 1]
        return r

    def expected_pcm(self, first, N, count=None):
        """-> (pcm [N][bs][ch], bits [N]) of the row that starts at block `first`, 0 <= first."""
        want, wb = expected_range(self.pcm, self.obits, int(first), N)
        if count is not None:
            m = max(0, min(N, int(count)))
            want[m:] = 0; wb[m:] = 0
        return want, wb

    def expected_spec(self, first, N, count=None, lr=False):
        """-> (coef [C][N][bs], wc [N], bits [N]) of the row that starts at block `first`."""
        coef, wc, bits = np.zeros((self.ch, N, self.bs), np.float32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        m = N if count is None else max(0, min(N, int(count)))
        if 0 <= first <= self.K:
            m = max(0, min(m, self.K - first))
            coef[:, :m] = self.coef[first:first + m].transpose(1, 0, 2)
            wc[:m], bits[:m] = self.wc[first:first + m], self.obits[first:first + m]
        return (to_lr(coef) if lr else coef), wc, bits


# the shared streams, one File each per process: whichever family asks first pays for an oracle run, once
@functools.lru_cache(maxsize=None)
def oracle_file(bs, ch, q, sid, seed=11, n_blocks=ORACLE_BLOCKS):
    blocks, bits, _ = oracle_stream(bs, ch, q, sid, seed, n_blocks)
    return File(f"oracle {bs}x{ch} q{q:g}", bs, ch, blocks, bits)


@functools.lru_cache(maxsize=None)
def synth_file(bs, ch, seed=SYNTH_SEED, n_blocks=SYNTH_BLOCKS):
    blocks, bits = synth_stream(bs, ch, seed, n_blocks)
    return File(f"hand-assembled {bs}x{ch}", bs, ch, blocks, bits)


@functools.lru_cache(maxsize=None)
def geom_files(geom):
    """The Files of a geometry of seek_testlib.geometries(), in its order and under its names."""
    out = [oracle_file(bs, ch, q, sid) for bs, ch, q, sid in ORACLE_CASES if (bs, ch) == tuple(geom)]
    out += [synth_file(bs, ch) for bs, ch in SYNTH_CASES if (bs, ch) == tuple(geom)]
    assert [f.name for f in out] == [name for name, _, _, _ in geometries()[tuple(geom)]]
    return out


class Corpus:
    """Files of one geometry in both layouts, with the index of each.
    files: [File, or None for a file nobody reads: no payload bytes, an index row of the single entry (0, SEED0)].
    payloads / offs: per file, what the buffers hold in place of the file's own bytes / byte offsets (a damaged copy under the
    clean index; an index nobody vouches for).  states: one value for every RngState of the index, fill included, in place of the
    oracle's.  index_slack: entries per strided row beyond the longest file's K + 1.
    strided: host uint8 [F][stride], nbytes int32 [F], index [F][istride], count int32 [F]; {-1, 0} behind a closing entry.
    ragged: rpay uint8 [total + PAD], poffs / ioffs int64 [F + 1], ridx [sum (K_f + 1)], count."""

    def __init__(self, files, payloads=None, offs=None, states=None, index_slack=0):
        self.files, self.F = list(files), len(files)
        ref = next(f for f in self.files if f is not None)
        self.bs, self.ch = ref.bs, ref.ch
        none = np.zeros(0, np.uint8)
        self.payloads = [none if f is None else f.payload for f in self.files] if payloads is None else list(payloads)
        self.offs = [np.zeros(1, np.int64) if f is None else f.offs for f in self.files] if offs is None else list(offs)
        self.K = [0 if f is None else f.K for f in self.files]
        self.count = np.array(self.K, np.int32)
        self.nbytes = np.array([len(p) for p in self.payloads], np.int32)
        self.stride = (max(len(p) for p in self.payloads) + PAD + 15) & ~15
        self.istride = max(self.K) + 1 + index_slack
        self.host = np.zeros((self.F, self.stride), np.uint8)
        self.index = np.zeros((self.F, self.istride), INDEX_DTYPE)
        self.index["ByteOffs"] = -1
        for i, (f, p) in enumerate(zip(self.files, self.payloads)):
            self.host[i, :len(p)] = p
            self.index["ByteOffs"][i, :self.K[i] + 1] = self.offs[i]
            if states is None:
                self.index["RngState"][i, :self.K[i] + 1] = SEED0 if f is None else f.seeds
        if states is not None:
            self.index["RngState"] = states
        self.poffs = np.concatenate([[0], np.cumsum(self.nbytes.astype(np.int64))]).astype(np.int64)
        self.ioffs = np.concatenate([[0], np.cumsum(np.array(self.K, np.int64) + 1)]).astype(np.int64)
        self.rpay = np.concatenate(list(self.payloads) + [np.zeros(PAD, np.uint8)]).astype(np.uint8)
        self.ridx = np.concatenate([self.index[i, :self.K[i] + 1] for i in range(self.F)])
        self._dev = None

    def strided(self):
        return dict(host=self.host, nbytes=self.nbytes, index=self.index, count=self.count)

    def ragged(self):
        return dict(payload=self.rpay, poffs=self.poffs, index=self.ridx, ioffs=self.ioffs, blocks=self.count.copy())

    def to_device(self):
        """Both layouts as torch tensors on cuda:0, uploaded once: pay / nb / idx (int32 [F][2 istride]) / cnt, and
        rpay / poffs / ridx (int32 [2 entries]) / ioffs."""
        if self._dev is None:
            import torch
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
            self._dev = dict(pay=t(self.host), nb=t(self.nbytes), idx=t(self.index.view(np.int32).reshape(self.F, -1)), cnt=t(self.count),
                             rpay=t(self.rpay), poffs=t(self.poffs), ridx=t(self.ridx.view(np.int32)), ioffs=t(self.ioffs))
        return self._dev

    def expected_pcm(self, files, first, N, count=None):
        """-> (pcm [n][N][bs][ch], bits [n][N]) of the rows; a file number outside the corpus, or a None file, gives zeros."""
        pcm = np.zeros((len(files), N, self.bs, self.ch), np.float32)
        bits = np.zeros((len(files), N), np.int32)
        for i, f in enumerate(files):
            if 0 <= f < self.F and self.files[f] is not None and 0 <= first[i] <= self.files[f].K:
                pcm[i], bits[i] = self.files[f].expected_pcm(first[i], N, None if count is None else count[i])
        return pcm, bits

    def expected_spec(self, files, first, N, count=None, lr=False):
        """-> (coef [n][C][N][bs], wc [n][N], bits [n][N]); a file number outside the corpus, or a None file, gives a row of zeros."""
        n = len(files)
        coef, wc, bits = np.zeros((n, self.ch, N, self.bs), np.float32), np.zeros((n, N), np.int32), np.zeros((n, N), np.int32)
        for i in range(n):
            if 0 <= files[i] < self.F and self.files[files[i]] is not None:
                coef[i], wc[i], bits[i] = self.files[files[i]].expected_spec(int(first[i]), N, None if count is None else count[i], lr)
        return coef, wc, bits
