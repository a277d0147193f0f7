"""A corpus of `.ulc` files resident in device memory, and random crops of it (ulcx_decode_crops_dev): what a loader holds.

    corpus = CropCorpus(n_chan=2, block_size=2048)
    for ulc, ulx in files:                         # bytes of the .ulc file and of its .ulx sidecar (or None: indexed in freeze)
        corpus.add_file(ulc, ulx)
    corpus.freeze("cuda:0")                        # payloads and indices to the device, once
    dec = ulc_amd.BatchDecoder(batch, 2, 2048, crop_blocks + 1)
    pcm, bits = corpus.crops(dec, files, first, crop_blocks)      # [n][crop_blocks * 2048][2] on the device
    pcm, bits = corpus.sample_crops(dec, files, start, n_samples) # [n][2][n_samples]: n_samples from sample start[i], channels-first
                                                                  # (dec: max_blocks > ulc_amd.crop_blocks(2048, n_samples))
    coef, wc, bits = corpus.spectra(dec, files, first, n_blocks)  # [n][2][n_blocks][2048]: the dequantised MDCT coefficients
    pcm, live = synth_spectra(dec, coef, wc, warm=True)           # and back: [n][2][(n_blocks - 1) * 2048], plane 0 the block in front
    dist, wc, bits = corpus.distortion(dec, files, first, n_blocks, ref, n_seg=8)   # [n][2][n_blocks][8][3] float64 {S, Y, E}: the coded
                                                                  # spectrum summed against reference planes; rung_plan() turns a ladder's into a plan

CropCorpus(..., layout="ragged") keeps every file at its own length (payloads and index rows back to back behind offset tables,
ulcx_decode_crops_ragged_dev) instead of at the longest file's: the layout for a corpus of files of very different length.

Everything in front of freeze() is host logic (numpy, and the library's host-side parsers): it needs no GPU.  Plumbing only -
the decode is the library's crop call, and there is no fallback."""
import ctypes as C
import numpy as np
import ulc_amd
from ulc_amd import INDEX_DTYPE, UlcError

ULC_HEADER_BYTES = 24
PAYLOAD_PAD = 64                                           # bytes behind the longest payload, as the tests' pack() leaves


def parse_ulc(data):
    """-> (FileHeader, payload bytes) of a `.ulc` file's bytes (ulcx_ulc_header_parse); raises UlcError on a foreign or short file."""
    h = ulc_amd.FileHeader()
    head = (C.c_uint8 * ULC_HEADER_BYTES).from_buffer_copy(bytes(data[:ULC_HEADER_BYTES]).ljust(ULC_HEADER_BYTES, b"\0"))
    ulc_amd._check(ulc_amd.lib().ulcx_ulc_header_parse(C.byref(h), head, min(len(data), ULC_HEADER_BYTES)), "ulcx_ulc_header_parse")
    if h.StreamOffs < ULC_HEADER_BYTES or h.StreamOffs > len(data):
        raise UlcError(f"ulc: the payload starts at byte {h.StreamOffs} of a file of {len(data)}")
    return h, bytes(data[h.StreamOffs:])


def sample_rows(start, length, block_size):
    """The block rows of sample crops, as the library's prologue kernel derives them (pure numpy; the tests hold the two together):
    start int64 [n] sample positions in the decoded streams, length [n] samples wanted (already clamped to [0, n_samples]).
    -> (first, count, skip) int64 [n]: the crop starts `skip` samples into block `first` and touches `count` blocks (0 for an
    empty row).  A negative start is refused as the library refuses it: first -1, count 0, skip 0."""
    start = np.asarray(start, np.int64)
    length = np.asarray(length, np.int64)
    bs = int(block_size)
    ok = start >= 0
    first = np.where(ok, start // bs, -1)
    skip = np.where(ok, start % bs, 0)
    count = np.where(ok & (length > 0), (skip + length - 1) // bs + 1, 0)
    return first, count, skip


def clip_spectra(enc, wave, lengths=None, n_blocks=None, lr=False):
    """The encoder's own MDCT coefficients of clips, without encoding them (ulcx_analyse_clips_dev): wave is a torch tensor
    [n][C][T], float32 or int16, row i the clip wave[i, :, :lengths[i]] (lengths as from_clips takes them), each analysed from a
    fresh state.  -> (coef float32 [n][C][n_blocks][BS], wc int32 [n][n_blocks], cplx float32 [n][n_blocks]) on wave's device,
    enqueued on torch's current stream: the normalised coefficients of the mid / side channels (lr: left / right, m + s and m - s)
    under the encoder's window code of that block - the layout of CropCorpus.spectra() - and zeros behind a row's last block.
    n_blocks: the planes' depth (default: what holds T samples).  enc: a BatchEncoder with n_streams >= n; no slot of it changes."""
    import torch
    n, ch, T = wave.shape
    if ch != enc.C:
        raise UlcError(f"clip spectra: clips of {ch} channels, an encoder of {enc.BS} x {enc.C}")
    dev = wave.device
    pcm16 = wave.dtype == torch.int16
    wave = wave.contiguous() if pcm16 else wave.to(torch.float32).contiguous()
    want = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32, device=dev).contiguous()
    depth = ulc_amd.clip_blocks(enc.BS, T) if n_blocks is None else int(n_blocks)
    coef, wc, cplx = _spectra_planes(n, ch, depth, enc.BS, dev)
    with torch.cuda.device(dev):
        enc.analyse_clips_dev(n, wave.data_ptr(), _ptr(want), T, depth, coef.data_ptr(), wc.data_ptr(), cplx.data_ptr(),
                              flags=ulc_amd.SPECTRA_LR if lr else 0, stream=torch.cuda.current_stream(dev).cuda_stream, pcm16=pcm16)
    return coef, wc, cplx


def synth_spectra(dec, coef, wc, *, lr=False, warm=False, pcm16=False):
    """PCM from MDCT planes held in torch tensors, through the decoder's own inverse transform (ulcx_synth_spectra_dev): coef float32
    [n][C][n_blocks][BS] and wc int32 [n][n_blocks] on one device, as CropCorpus.spectra(), clip_spectra() and from_clips_spectra()
    leave them - the window codes must come with the planes.  -> (pcm [n][C][n_out * BS] float32, or int16 with pcm16; live int32
    [n][n_out]) on that device, enqueued on torch's current stream.  warm: plane 0 of every row is the block in front of the output
    (n_out = n_blocks - 1, else n_blocks); lr: the planes hold left / right, nothing is un-mixed.  Contiguous input is not copied.
    dec: a BatchDecoder with n_streams >= n and max_blocks > n_out; no stream of it changes."""
    import torch
    if coef.dim() != 4 or wc.dim() != 2:
        raise UlcError(f"synth spectra: planes of {coef.dim()} dimensions and codes of {wc.dim()} ([n][C][n_blocks][BS] and [n][n_blocks])")
    n, ch, depth, bs = coef.shape
    if ch != dec.C or bs != dec.BS:
        raise UlcError(f"synth spectra: planes of {bs} x {ch}, a decoder of {dec.BS} x {dec.C}")
    if tuple(wc.shape) != (n, depth):
        raise UlcError(f"synth spectra: codes {tuple(wc.shape)} beside planes of {n} rows x {depth} blocks")
    if coef.dtype != torch.float32 or wc.dtype != torch.int32:
        raise UlcError(f"synth spectra: planes {coef.dtype} (float32), codes {wc.dtype} (int32)")
    if wc.device != coef.device or not coef.is_cuda:
        raise UlcError(f"synth spectra: planes on {coef.device}, codes on {wc.device} (one GPU)")
    n_out = depth - (1 if warm else 0)
    if n < 1 or n_out < 1:
        raise UlcError(f"synth spectra: {n} rows of {n_out} output blocks")
    dev = coef.device
    coef = coef.contiguous()
    wc = wc.contiguous()
    pcm = torch.empty((n, ch, n_out * bs), dtype=torch.int16 if pcm16 else torch.float32, device=dev)
    live = torch.empty((n, n_out), dtype=torch.int32, device=dev)
    flags = (ulc_amd.SPECTRA_LR if lr else 0) | (ulc_amd.SYNTH_WARM if warm else 0)
    with torch.cuda.device(dev):
        dec.synth_spectra_dev(n, depth, flags, coef.data_ptr(), wc.data_ptr(), pcm.data_ptr(), live.data_ptr(),
                              stream=torch.cuda.current_stream(dev).cuda_stream, pcm16=pcm16)
    return pcm, live


def _ptr(t):
    """A tensor's device address for the library; 0 for None: not given."""
    return t.data_ptr() if t is not None else 0


def _empty_strided(n_files, stride, index_stride, dev):
    """Unwritten tensors of a strided corpus -> (payload, stride, payload_bytes, index, index_stride, index_blocks), the order the
    library's calls and _adopt() take them in."""
    import torch
    return (torch.empty((n_files, stride), dtype=torch.uint8, device=dev), stride, torch.empty(n_files, dtype=torch.int32, device=dev),
            torch.empty((n_files, index_stride, 2), dtype=torch.int32, device=dev), index_stride, torch.empty(n_files, dtype=torch.int32, device=dev))


def _corpus_ptrs(strided):
    return tuple(_ptr(v) if hasattr(v, "data_ptr") else v for v in strided)


def _spectra_planes(n, ch, depth, block_size, dev):
    import torch
    if depth < 1:
        raise UlcError(f"clip spectra: n_blocks {depth}")
    return (torch.empty((n, ch, depth, block_size), dtype=torch.float32, device=dev), torch.empty((n, depth), dtype=torch.int32, device=dev),
            torch.empty((n, depth), dtype=torch.float32, device=dev))


class CropCorpus:
    def __init__(self, n_chan, block_size, layout="strided"):
        if layout not in ("strided", "ragged"):
            raise UlcError(f"corpus: layout {layout!r} (strided or ragged)")
        self.C, self.BS, self.ragged = int(n_chan), int(block_size), layout == "ragged"
        self._payloads, self._index, self._blocks = [], [], []      # per file: bytes; entries [n + 1] or None; blocks (header's when not indexed yet)
        self.frozen = False

    def __len__(self):
        return self.n_files if self.frozen else len(self._payloads)

    @classmethod
    def from_clips_spectra(cls, enc, dec, wave, lengths=None, rate=(ulc_amd.MODE_VBR, 50.0), layout="strided", payload_stride=None,
                           n_blocks=None, lr=False):
        """from_clips() with the tap (ulcx_encode_clips_spectra_dev) -> (corpus, coef, wc, cplx): the same corpus, and the clean
        spectra of the same blocks as clip_spectra() returns them, out of the same pass.  corpus.spectra(dec, arange(n), zeros(n),
        n_blocks) then gives the coded spectra on the same grid: block k of row i pairs up for every k below the file's block count."""
        return cls.from_clips(enc, dec, wave, lengths, rate, layout, payload_stride, _tap=(n_blocks, lr))

    @classmethod
    def from_clips(cls, enc, dec, wave, lengths=None, rate=(ulc_amd.MODE_VBR, 50.0), layout="strided", payload_stride=None, _tap=None):
        """A frozen corpus straight from waveforms on the device (ulcx_encode_clips_dev): wave is a torch tensor [n][C][T], float32
        or int16, row i the clip wave[i, :, :lengths[i]] (lengths: int32 [n] on the device or anything torch.as_tensor takes; None:
        every row T samples), each encoded from a fresh state.  rate: (mode, p0[, p1]) for every row, or a float32 [n][2] table
        {RateKbps, AvgComplexity} in the tool's convention.  enc: a BatchEncoder with n_streams >= n (none of its slots is read or
        changed); dec: a BatchDecoder of the same geometry.  Everything is enqueued on torch's current stream and the corpus adopts
        the tensors the call wrote: no host trip and no freeze().  payload_stride: bytes per file of the strided layout (default:
        what always suffices, slot bytes x blocks of T samples; a row that does not fit keeps its leading blocks).
        layout="ragged" runs ulcx_corpus_ragged_dev behind it; sizing the ragged buffers takes ONE 16-byte read of the totals."""
        import torch
        c, n, T, dev, pcm16, wave, want = cls._clips_in(enc, dec, wave, lengths, layout)
        table = None
        mode, p0, p1 = ulc_amd.MODE_VBR, 50.0, 0.0
        if isinstance(rate, tuple):
            mode, p0, p1 = int(rate[0]), float(rate[1]), float(rate[2]) if len(rate) > 2 else 0.0
        else:
            table = torch.as_tensor(rate, dtype=torch.float32, device=dev).contiguous()
            assert tuple(table.shape) == (n, 2)
        nb, stream, out = cls._clips_out(enc, n, T, payload_stride, dev)
        planes = None
        if _tap is not None:
            depth = nb if _tap[0] is None else int(_tap[0])
            planes = _spectra_planes(n, enc.C, depth, enc.BS, dev)
        with torch.cuda.device(dev):
            args = (dec, n, wave.data_ptr(), _ptr(want), T, *_corpus_ptrs(out))
            kw = dict(mode=mode, p0=p0, p1=p1, d_rates=_ptr(table), stream=stream, pcm16=pcm16)
            if planes is None:
                enc.encode_clips_dev(*args, **kw)
            else:
                enc.encode_clips_spectra_dev(*args, depth, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
                                             flags=ulc_amd.SPECTRA_LR if _tap[1] else 0, **kw)
            c._adopt(dev, stream, n, *out)
        c.frozen = True
        return c if planes is None else (c, *planes)

    @classmethod
    def _clips_in(cls, enc, dec, wave, lengths, layout):
        """What the clip calls share in front of their rates: the geometry check, the corpus object, wave and lengths as the call
        reads them -> (corpus, n, T, device, pcm16, wave, lengths or None)."""
        import torch
        n, ch, T = wave.shape
        if (ch, enc.BS) != (dec.C, dec.BS) or ch != enc.C:
            raise UlcError(f"corpus: clips of {ch} channels, an encoder of {enc.BS} x {enc.C}, a decoder of {dec.BS} x {dec.C}")
        c = cls(ch, enc.BS, layout)
        dev = wave.device
        pcm16 = wave.dtype == torch.int16
        wave = wave.contiguous() if pcm16 else wave.to(torch.float32).contiguous()
        want = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32, device=dev).contiguous()
        return c, n, T, dev, pcm16, wave, want

    @staticmethod
    def _clips_out(enc, n_files, T, payload_stride, dev):
        """And behind them: what the call writes -> (blocks of T samples, torch's current stream, _empty_strided() of n_files files
        at the default strides, which hold every file in full, unless payload_stride is given)."""
        import torch
        nb = ulc_amd.clip_blocks(enc.BS, T)
        return nb, torch.cuda.current_stream(dev).cuda_stream, _empty_strided(n_files, int(payload_stride or enc.slot * nb), nb + 1, dev)

    def _adopt(self, dev, stream, n, payload, stride, nbytes, index, index_stride, blocks):
        """The tensors a clips call wrote (n files, strided) become the corpus's; a ragged corpus lays them out with
        ulcx_corpus_ragged_dev on `stream` first.  Called inside torch.cuda.device(dev)."""
        import torch
        self.n_files, self.device = n, dev
        if not self.ragged:
            self.stride, self.index_stride = stride, index_stride
            self.d_payload, self.d_payload_bytes, self.d_index, self.d_index_blocks = payload, nbytes, index, blocks
            return
        poffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ioffs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        oblocks = torch.empty(n, dtype=torch.int32, device=dev)
        need = torch.empty(2, dtype=torch.int64, device=dev)
        none = torch.empty(16, dtype=torch.uint8, device=dev)
        args = (n, *_corpus_ptrs((payload, stride, nbytes, index, index_stride, blocks)))
        ulc_amd.corpus_ragged_dev(*args, none.data_ptr(), 0, poffs.data_ptr(), none.data_ptr(), 0, ioffs.data_ptr(), oblocks.data_ptr(),
                                  need.data_ptr(), stream=stream, device=dev.index or 0)
        nbytes_all, nent_all = (int(v) for v in need.cpu())
        opay = torch.empty(nbytes_all + PAYLOAD_PAD, dtype=torch.uint8, device=dev)
        oidx = torch.empty((max(1, nent_all), 2), dtype=torch.int32, device=dev)
        ulc_amd.corpus_ragged_dev(*args, opay.data_ptr(), nbytes_all, poffs.data_ptr(), oidx.data_ptr(), nent_all, ioffs.data_ptr(), oblocks.data_ptr(),
                                  need.data_ptr(), stream=stream, device=dev.index or 0)
        self.d_payload, self.d_payload_offs, self.d_index, self.d_index_offs, self.d_index_blocks = opay, poffs, oidx, ioffs, oblocks
        # (the strided tensors go back to torch's allocator, which hands them out again on this stream only: behind the copy)

    @classmethod
    def from_clips_ladder(cls, enc, dec, wave, lengths=None, rates=((ulc_amd.MODE_VBR, 50.0),), layout="strided", payload_stride=None):
        """from_clips() under several rates in one call (ulcx_encode_clips_ladder_dev) -> ONE frozen corpus of R * n files: file
        corpus.file_of(rung, clip) = rung * n + clip is that clip under rates[rung].  A rate is (mode, p0[, p1]) for every clip,
        ("auto", kbps) - the clip in ABR at kbps and at its OWN average block complexity, the tool's two-run `RATE,auto`, with the
        analysis pass on the device - or a float32 [n][2] table {RateKbps, AvgComplexity} per clip; ("auto_table", table) puts each
        clip's own average in the table's second column.  corpus.avg is then a float32 [n] tensor of the clips' averages (None
        without an "auto" rate); corpus.n_rungs and corpus.n_clips are R and n.  At most ulc_amd.MAX_RUNGS rates; enc, dec, wave,
        lengths, layout and payload_stride (bytes per FILE) as from_clips takes them."""
        import numbers
        import torch
        rates = list(rates)
        R = len(rates)
        c, n, T, dev, pcm16, wave, want = cls._clips_in(enc, dec, wave, lengths, layout)
        tables = []                                        # (alive until the call is enqueued; torch frees them in stream order)

        def table_ptr(r, t):
            t = torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
            if tuple(t.shape) != (n, 2):
                raise UlcError(f"corpus: rate {r}: a table of shape {tuple(t.shape)} for {n} clips ([n][2] = RateKbps, AvgComplexity per clip)")
            tables.append(t)
            return t.data_ptr()
        number = lambda x: isinstance(x, numbers.Real) and not isinstance(x, bool)
        rungs = []
        for r, g in enumerate(rates):
            # a scalar rate is a tuple of 2 or 3 numbers, or ("auto", number); anything else must be a table [n][2] - a table
            # written as a tuple of rows included
            if isinstance(g, tuple) and len(g) == 2 and g[0] == "auto_table":
                rungs.append(("auto_table", table_ptr(r, g[1])))
            elif isinstance(g, tuple) and len(g) == 2 and g[0] == "auto" and number(g[1]):
                rungs.append(("auto", float(g[1])))
            elif isinstance(g, tuple) and len(g) in (2, 3) and all(number(x) for x in g):
                rungs.append(g)
            elif isinstance(g, tuple) and len(g) and isinstance(g[0], str):
                raise UlcError(f"corpus: rate {r}: {g!r} ((mode, p0[, p1]), ('auto', kbps), ('auto_table', table) or a table)")
            else:
                rungs.append(table_ptr(r, g))
        auto = any(isinstance(g, tuple) and g[0] in ("auto", "auto_table") for g in rungs)
        _, stream, out = cls._clips_out(enc, max(R, 1) * n, T, payload_stride, dev)
        avg = torch.empty(n, dtype=torch.float32, device=dev) if auto else None
        with torch.cuda.device(dev):
            enc.encode_clips_ladder_dev(dec, n, rungs, wave.data_ptr(), _ptr(want), T, *_corpus_ptrs(out), d_avg=_ptr(avg), stream=stream, pcm16=pcm16)
            c._adopt(dev, stream, max(R, 1) * n, *out)
        c.n_rungs, c.n_clips, c.avg = R, n, avg
        c.frozen = True
        return c

    def file_of(self, rung, clip):
        """The file number of `clip` under rate `rung` in a corpus from_clips_ladder() made."""
        if not hasattr(self, "n_rungs"):
            raise UlcError("corpus: file_of() is for a corpus that from_clips_ladder() made")
        if not (0 <= rung < self.n_rungs and 0 <= clip < self.n_clips):
            raise UlcError(f"corpus: rung {rung}, clip {clip} of {self.n_rungs} x {self.n_clips}")
        return rung * self.n_clips + clip

    def add_file(self, ulc_bytes, ulx_bytes=None):
        """-> the file's number.  Refuses (UlcError) another geometry than the corpus's, and a `.ulx` that is not this payload's:
        another geometry, another PayloadBytes, or entries ulcx_index_check does not accept for it.  Without `.ulx` bytes the
        file is marked for indexing in freeze()."""
        if self.frozen:
            raise UlcError("corpus: frozen")
        h, payload = parse_ulc(ulc_bytes)
        if (h.BlockSize, h.nChan) != (self.BS, self.C):
            raise UlcError(f"corpus: a file of BlockSize {h.BlockSize} x {h.nChan} channels in a corpus of {self.BS} x {self.C}")
        if len(payload) < 1 or len(payload) >= 2 ** 31 - PAYLOAD_PAD - 16:
            raise UlcError(f"corpus: a payload of {len(payload)} bytes")
        entries, blocks = None, max(1, int(h.nBlocks))
        if ulx_bytes is not None:
            xh, entries = ulc_amd.ulx_parse(ulx_bytes)
            if (xh.BlockSize, xh.nChan) != (self.BS, self.C):
                raise UlcError(f"corpus: an index of BlockSize {xh.BlockSize} x {xh.nChan} channels in a corpus of {self.BS} x {self.C}")
            if xh.PayloadBytes != len(payload):
                raise UlcError(f"corpus: the index was made for a payload of {xh.PayloadBytes} bytes, the file's has {len(payload)}")
            if not ulc_amd.index_check(entries, xh.nBlocks, len(payload)):
                raise UlcError("corpus: the index does not fit the payload (ulcx_index_check)")
            blocks = int(xh.nBlocks)
        self._payloads.append(payload); self._index.append(entries); self._blocks.append(blocks)
        return len(self._payloads) - 1

    def layout(self):
        """The frozen layout on numpy arrays: one stride for the payloads (the longest + 64, rounded up to 16), one for the
        indices (the most blocks + 1); file f's payload starts at byte f * stride.  -> dict: stride, index_stride, payload uint8
        [F][stride], payload_bytes int32 [F], index INDEX_DTYPE [F][index_stride] (an open row, ulc_amd.new_index, for a file to
        index), index_blocks int32 [F] (0 for those), to_index: the numbers of the files without a stored index."""
        F = len(self._payloads)
        if F < 1:
            raise UlcError("corpus: no files")
        if self.ragged:
            return self._layout_ragged()
        stride = (max(len(p) for p in self._payloads) + PAYLOAD_PAD + 15) & ~15
        index_stride = max(self._blocks) + 1
        payload = np.zeros((F, stride), np.uint8)
        nbytes = np.zeros(F, np.int32)
        index = ulc_amd.new_index(F, index_stride)
        blocks = np.zeros(F, np.int32)
        for f, (p, e) in enumerate(zip(self._payloads, self._index)):
            payload[f, :len(p)] = np.frombuffer(p, np.uint8)
            nbytes[f] = len(p)
            if e is not None:
                index[f, :len(e)] = e
                blocks[f] = len(e) - 1
        to_index = np.array([f for f, e in enumerate(self._index) if e is None], np.int64)
        return {"stride": stride, "index_stride": index_stride, "payload": payload, "payload_bytes": nbytes, "index": index,
                "index_blocks": blocks, "to_index": to_index}

    def _layout_ragged(self):
        """layout() of a ragged corpus: the payloads back to back with PAYLOAD_PAD bytes behind the last one, row f of the index
        with blocks_f + 1 entries.  -> dict: payload uint8 [total], payload_offs int64 [F + 1] (file f is bytes offs[f] ..
        offs[f + 1]), index INDEX_DTYPE [entries], index_offs int64 [F + 1], index_blocks, to_index as above."""
        F = len(self._payloads)
        poffs = np.zeros(F + 1, np.int64)
        poffs[1:] = np.cumsum([len(p) for p in self._payloads])
        ioffs = np.zeros(F + 1, np.int64)
        ioffs[1:] = np.cumsum([b + 1 for b in self._blocks])
        payload = np.zeros(int(poffs[-1]) + PAYLOAD_PAD, np.uint8)
        index = np.zeros(int(ioffs[-1]), INDEX_DTYPE)
        blocks = np.zeros(F, np.int32)
        for f, (p, e) in enumerate(zip(self._payloads, self._index)):
            payload[poffs[f]:poffs[f + 1]] = np.frombuffer(p, np.uint8)
            if e is not None:
                index[ioffs[f]:ioffs[f + 1]] = e
                blocks[f] = len(e) - 1
            else:
                index[ioffs[f]:ioffs[f + 1]] = ulc_amd.new_index(1, self._blocks[f] + 1)[0]
        to_index = np.array([f for f, e in enumerate(self._index) if e is None], np.int64)
        return {"payload": payload, "payload_offs": poffs, "index": index, "index_offs": ioffs, "index_blocks": blocks, "to_index": to_index}

    def _freeze_ragged(self, dev):
        """freeze() of a ragged corpus: the files without a stored index are indexed with ONE ulcx_index_packed_ragged_dev call - in
        place when that is every file, else on a copy of those files' payloads, whose rows then go to their places."""
        import torch
        lay = self.layout()
        F = self.n_files = len(self._payloads)
        self.device = dev
        self.d_payload = torch.from_numpy(lay["payload"]).to(dev)
        self.d_payload_offs = torch.from_numpy(lay["payload_offs"]).to(dev)
        self.d_index = torch.from_numpy(lay["index"].view(np.int32).reshape(-1, 2)).to(dev)
        self.d_index_offs = torch.from_numpy(lay["index_offs"]).to(dev)
        self.d_index_blocks = torch.from_numpy(lay["index_blocks"]).to(dev)
        todo = lay["to_index"]
        if todo.size:
            poffs, ioffs = lay["payload_offs"], lay["index_offs"]
            if todo.size == F:
                pay, po, idx, io, cnt, dst = self.d_payload, self.d_payload_offs, self.d_index, self.d_index_offs, self.d_index_blocks, None
            else:
                sub = np.concatenate([lay["payload"][poffs[f]:poffs[f + 1]] for f in todo] + [np.zeros(PAYLOAD_PAD, np.uint8)])
                caps = np.array([ioffs[f + 1] - ioffs[f] for f in todo], np.int64)
                pay = torch.from_numpy(sub).to(dev)
                po = torch.from_numpy(np.concatenate([[0], np.cumsum([poffs[f + 1] - poffs[f] for f in todo])]).astype(np.int64)).to(dev)
                io = torch.from_numpy(np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)).to(dev)
                idx = torch.zeros((int(caps.sum()), 2), dtype=torch.int32, device=dev)
                cnt = torch.zeros(todo.size, dtype=torch.int32, device=dev)
                dst = torch.from_numpy(np.concatenate([np.arange(ioffs[f], ioffs[f + 1]) for f in todo])).to(dev)
            with torch.cuda.device(dev):
                dec = ulc_amd.BatchDecoder(1, self.C, self.BS, 1, device=dev.index or 0)     # geometry and tables are all the call reads of it
                try:
                    dec.index_packed_ragged_dev(int(todo.size), pay.data_ptr(), pay.numel(), po.data_ptr(), idx.data_ptr(), idx.shape[0], io.data_ptr(),
                                                cnt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
                    torch.cuda.current_stream(dev).synchronize()
                finally:
                    dec.close()
            if dst is not None:
                self.d_index.index_copy_(0, dst, idx)
                self.d_index_blocks.index_copy_(0, torch.from_numpy(todo).to(dev), cnt)
        self.frozen = True
        return self

    def freeze(self, device="cuda:0"):
        """Payloads and indices to `device` as torch tensors (uint8 / int32), at the strides of layout(); the files without a
        stored index are indexed there with ONE ulcx_index_packed_rows_dev call.  (A ragged corpus: _freeze_ragged.)"""
        import torch
        dev = torch.device(device)
        if self.ragged:
            return self._freeze_ragged(dev)
        lay = self.layout()
        self.n_files, self.stride, self.index_stride = len(self._payloads), lay["stride"], lay["index_stride"]
        self.device = dev
        self.d_payload = torch.from_numpy(lay["payload"]).to(dev)
        self.d_payload_bytes = torch.from_numpy(lay["payload_bytes"]).to(dev)
        self.d_index = torch.from_numpy(lay["index"].view(np.int32).reshape(self.n_files, self.index_stride, 2)).to(dev)
        self.d_index_blocks = torch.from_numpy(lay["index_blocks"]).to(dev)
        todo = lay["to_index"]
        if todo.size:
            rows = torch.from_numpy(todo).to(dev)
            pay = self.d_payload.index_select(0, rows).contiguous()
            nb = self.d_payload_bytes.index_select(0, rows).contiguous()
            idx = torch.zeros((todo.size, self.index_stride, 2), dtype=torch.int32, device=dev)
            cnt = torch.zeros(todo.size, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                dec = ulc_amd.BatchDecoder(1, self.C, self.BS, 1, device=dev.index or 0)     # geometry and tables are all the call reads of it
                try:
                    dec.index_packed_rows_dev(int(todo.size), pay.data_ptr(), self.stride, nb.data_ptr(), self.index_stride - 1, idx.data_ptr(),
                                              cnt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
                    torch.cuda.current_stream(dev).synchronize()
                finally:
                    dec.close()
            self.d_index.index_copy_(0, rows, idx)
            self.d_index_blocks.index_copy_(0, rows, cnt)
        self.frozen = True
        return self

    def device_bytes(self):
        """HBM bytes of the frozen corpus: payloads, their sizes (ragged: the two offset tables), indices, block counts."""
        held = ((self.d_payload, self.d_payload_offs, self.d_index, self.d_index_offs, self.d_index_blocks) if self.ragged else
                (self.d_payload, self.d_payload_bytes, self.d_index, self.d_index_blocks))
        return sum(t.numel() * t.element_size() for t in held)

    def crops(self, dec, files, first, n_blocks, count=None, pcm16=False):
        """Row i: blocks first[i] .. first[i] + n_blocks - 1 of file files[i] (the leading count[i] of them when `count` is
        given; zeros behind).  files / first / count: int32 tensors on the corpus's device, or anything torch.as_tensor takes.
        -> (pcm [n][n_blocks * BlockSize][nChan] float32, or int16 with pcm16; bits int32 [n][n_blocks]) on the device, enqueued on
        torch's current stream.  `dec`: a BatchDecoder of this geometry with n_streams >= n and max_blocks > n_blocks; no stream
        state of it is read or changed."""
        import torch
        sfx, corpus = self._ready(dec)._view()
        n, files, first, want = self._rows(files, first, count)
        pcm = torch.empty((n, n_blocks * self.BS, self.C), dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        bits = torch.empty((n, n_blocks), dtype=torch.int32, device=self.device)
        getattr(dec, f"decode_crops{sfx}_dev")(*corpus, n, files.data_ptr(), first.data_ptr(), _ptr(want), n_blocks, pcm.data_ptr(), bits.data_ptr(),
                                               stream=torch.cuda.current_stream(self.device).cuda_stream, pcm16=pcm16)
        return pcm, bits

    def _ready(self, dec):
        """Refuses a corpus that is not frozen and a decoder of another geometry -> self."""
        if not self.frozen:
            raise UlcError("corpus: not frozen")
        if (dec.C, dec.BS) != (self.C, self.BS):
            raise UlcError(f"corpus: a decoder of {dec.BS} x {dec.C} for a corpus of {self.BS} x {self.C}")
        return self

    def _view(self):
        """The frozen corpus as a device form takes it -> (the suffix of the form's name: decode_crops<suffix>_dev, the arguments
        n_files .. d_index_blocks of that form)."""
        if self.ragged:
            return "_ragged", (self.n_files, self.d_payload.data_ptr(), self.d_payload.numel(), self.d_payload_offs.data_ptr(), self.d_index.data_ptr(),
                               self.d_index.shape[0], self.d_index_offs.data_ptr(), self.d_index_blocks.data_ptr())
        return "", (self.n_files, self.d_payload.data_ptr(), self.stride, self.d_payload_bytes.data_ptr(), self.d_index.data_ptr(), self.index_stride,
                    self.d_index_blocks.data_ptr())

    def _rows(self, files, pos, want, *more, pos_dtype=None):
        """The rows of a crop call as contiguous tensors on the corpus's device -> (n, files, pos, want, *more): files int32 [n],
        pos of pos_dtype (default int32), want and `more` int32 [n] or None.  The caller holds them until its call is enqueued."""
        import torch
        as_t = lambda v, t=torch.int32: torch.as_tensor(v, dtype=t, device=self.device).contiguous()
        files, pos = as_t(files), as_t(pos, pos_dtype or torch.int32)
        opt = [None if v is None else as_t(v) for v in (want, *more)]
        n = files.numel()
        assert pos.numel() == n and all(v is None or v.numel() == n for v in opt)
        return (n, files, pos, *opt)

    def splice(self, dec, segments):
        """A new corpus whose files are block ranges of this one's (ulcx_corpus_splice_dev): rung switches, trims, joins.
        `segments` is one list of (file, first, count) per output file - output file o is those ranges back to back, in order - or
        the tuple (file, first, count, offs): three int32 [nSeg] tensors and the int32 [nOut + 1] offsets of each output file's
        segments among them.  Positions are whole blocks; an output file stops in front of the first block that cannot be taken.
        -> (corpus, seg_start): a frozen CropCorpus on the device in this corpus's layout (strided; ragged: ulcx_corpus_ragged_dev
        behind the call), sized from this corpus's index (ONE 16-byte read of the largest planned file), and the int32 [nSeg]
        output block at which each segment begins in its file.  Enqueued on torch's current stream.  `dec`: a BatchDecoder of this
        geometry; geometry and tables are all the call reads of it."""
        import torch
        sfx, corpus = self._ready(dec)._view()
        dev = self.device
        as_i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=dev).contiguous()
        if isinstance(segments, tuple):
            file, first, count, offs = (as_i32(v).reshape(-1) for v in segments)
        else:
            flat = np.array([tuple(g) for f in segments for g in f], np.int32).reshape(-1, 3)
            file, first, count = (as_i32(flat[:, j].copy()) for j in range(3))
            offs = as_i32(np.concatenate([[0], np.cumsum([len(f) for f in segments])]))
        n_out, n_seg = offs.numel() - 1, file.numel()
        if n_out < 1 or n_seg < 1 or first.numel() != n_seg or count.numel() != n_seg:
            raise UlcError(f"corpus: a splice of {n_out} files from {n_seg} segments")
        seg = torch.stack((file, first, count), dim=1).contiguous()
        # the plan's size from the index: per segment the blocks and bytes its range holds, summed per output file
        F = self.n_files
        f = file.long().clamp(0, F - 1)
        if self.ragged:
            i0 = self.d_index_offs[:-1]
            n_i = torch.minimum(self.d_index_blocks.long().clamp(min=0), (self.d_index_offs[1:] - i0 - 1).clamp(min=0))[f]
            at = lambda k: self.d_index[:, 0][(i0[f] + k).clamp(0, max(self.d_index.shape[0] - 1, 0))]
        else:
            n_i = self.d_index_blocks.long().clamp(0, self.index_stride - 1)[f]
            at = lambda k: self.d_index[:, :, 0][f, k]
        a = torch.minimum(first.long().clamp(min=0), n_i)
        b = torch.minimum(a + count.long().clamp(min=0), n_i)
        size = torch.stack((b - a, (at(b) - at(a)).long().clamp(min=0)), dim=1)
        owner = (torch.searchsorted(offs.long(), torch.arange(n_seg, device=dev), right=True) - 1).clamp(0, n_out - 1)
        most = torch.zeros((n_out, 2), dtype=torch.int64, device=dev).index_add_(0, owner, size).amax(dim=0)
        n_blocks, n_bytes = (int(v) for v in most.cpu())
        stride = (n_bytes + PAYLOAD_PAD + 15) & ~15
        index_stride = n_blocks + 1 if n_blocks > 0 else 2
        out = _empty_strided(n_out, stride, index_stride, dev)
        seg_start = torch.empty(n_seg, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        payload, stride, nbytes, index, index_stride, blocks = _corpus_ptrs(out)
        c = CropCorpus(self.C, self.BS, "ragged" if self.ragged else "strided")
        with torch.cuda.device(dev):
            getattr(dec, f"corpus_splice{sfx}_dev")(*corpus, n_out, offs.data_ptr(), seg.data_ptr(), n_seg, payload, stride, nbytes, 0, index, index_stride,
                                                    blocks, seg_start.data_ptr(), stream=stream)
            c._adopt(dev, stream, n_out, *out)
        c.frozen = True
        return c, seg_start

    def trim(self, dec, first, count):
        """Every file cut to its blocks first[f] .. first[f] + count[f] - 1 (int32 [n_files], or anything torch.as_tensor takes;
        a scalar for all files) -> the new corpus, file for file (splice() with one segment per file)."""
        import torch
        n = self.n_files
        as_row = lambda v: torch.as_tensor(v, dtype=torch.int32, device=self.device).reshape(-1).expand(n).contiguous()
        every = torch.arange(n + 1, dtype=torch.int32, device=self.device)
        return self.splice(dec, (every[:n], as_row(first), as_row(count), every))[0]

    def switch(self, dec, plan):
        """Rung switching on a corpus from_clips_ladder() made: plan[clip] is a list of (rung, n_blocks) - output file `clip` takes
        n_blocks blocks of the clip under that rung, then goes on where it stands under the next one.  Every rung of a clip has the
        same window code in every block, so the aliasing cancels at each joint.  -> the new corpus of len(plan) files."""
        segments = []
        for clip, runs in enumerate(plan):
            at, row = 0, []
            for rung, n_blocks in runs:
                row.append((self.file_of(int(rung), clip), at, int(n_blocks)))
                at += int(n_blocks)
            segments.append(row)
        return self.splice(dec, segments)[0]

    def sample_crops(self, dec, files, start, n_samples, length=None, pcm16=False, lowrate=0, part=None):
        """Row i: n_samples samples from sample start[i] of the decoded stream of file files[i] (its leading length[i] when
        `length` is given; zeros behind, and behind the file's end), written channels-first by the synthesis itself
        (ulcx_decode_crops_samples_dev): no gather, no transpose.  start: int64; files / length: int32; tensors on the corpus's
        device, or anything torch.as_tensor takes.  Positions are of the decoded stream: the codec's delay is not compensated.
        -> (pcm [n][nChan][n_samples] float32, or int16 with pcm16; bits int32 [n][crop_blocks]) on the device, enqueued on
        torch's current stream.  `dec`: a BatchDecoder of this geometry with n_streams >= n and max_blocks > crop_blocks =
        ulc_amd.crop_blocks(BlockSize, n_samples); no stream state of it is read or changed.
        lowrate = 1, 2, 3: the crop at 1/2, 1/4, 1/8 of the file's rate straight from the synthesis (ulcx_decode_crops_lowrate_dev):
        start, length and n_samples count samples of the reduced stream - blocks of BlockSize >> lowrate, reduced sample m at
        full-rate time D m + (D - 1) / 2 with D = 1 << lowrate - and crop_blocks is that of the reduced BlockSize.  0: the
        full-rate call, untouched.
        part = "mid" / "side": one coded channel of every pair, as it stands in front of the decoder's un-mix
        (ulcx_decode_crops_part_dev; at any lowrate, 0 included) -> pcm [n][part_channels][n_samples]: plane j is coded channel 2 j
        (mid; an unpaired last channel is the last plane) or 2 j + 1 (side).  The mid of a stereo file is its mono downmix
        (L + R) / 2 as the file codes it - equal to the folded stereo decode up to the un-mix's two float32 roundings, not bit for
        bit.  None: the paths above, untouched."""
        import torch
        sfx, corpus = self._ready(dec)._view()
        n, files, start, want = self._rows(files, start, length, pos_dtype=torch.int64)
        if part is not None:
            if part not in ("mid", "side"):
                raise ValueError(f"part {part!r}: 'mid', 'side' or None")
            which = ulc_amd.PART_MID if part == "mid" else ulc_amd.PART_SIDE
            planes, bs = ulc_amd.part_channels(self.C, which), ulc_amd.lowrate_block(self.BS, lowrate)
            if not planes:
                raise ValueError(f"part {part!r}: {self.C} channel(s) have no side")
            if not bs:
                raise ValueError(f"lowrate {lowrate}: 0 .. 3 with BlockSize {self.BS} >> lowrate >= 256")
            pcm = torch.empty((n, planes, n_samples), dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
            bits = torch.empty((n, ulc_amd.crop_blocks(bs, n_samples)), dtype=torch.int32, device=self.device)
            getattr(dec, f"decode_crops_part{sfx}_dev")(*corpus, n, files.data_ptr(), start.data_ptr(), _ptr(want), n_samples, int(lowrate), which, pcm.data_ptr(),
                                                        bits.data_ptr(), stream=torch.cuda.current_stream(self.device).cuda_stream, pcm16=pcm16)
            return pcm, bits
        pcm = torch.empty((n, self.C, n_samples), dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        if lowrate:
            bs = ulc_amd.lowrate_block(self.BS, lowrate)
            if not bs:
                raise ValueError(f"lowrate {lowrate}: 0 .. 3 with BlockSize {self.BS} >> lowrate >= 256")
            bits = torch.empty((n, ulc_amd.crop_blocks(bs, n_samples)), dtype=torch.int32, device=self.device)
            getattr(dec, f"decode_crops_lowrate{sfx}_dev")(*corpus, n, files.data_ptr(), start.data_ptr(), _ptr(want), n_samples, int(lowrate), pcm.data_ptr(),
                                                           bits.data_ptr(), stream=torch.cuda.current_stream(self.device).cuda_stream, pcm16=pcm16)
            return pcm, bits
        bits = torch.empty((n, ulc_amd.crop_blocks(self.BS, n_samples)), dtype=torch.int32, device=self.device)
        getattr(dec, f"decode_crops_samples{sfx}_dev")(*corpus, n, files.data_ptr(), start.data_ptr(), _ptr(want), n_samples, pcm.data_ptr(), bits.data_ptr(),
                                                       stream=torch.cuda.current_stream(self.device).cuda_stream, pcm16=pcm16)
        return pcm, bits

    def spectra(self, dec, files, first, n_blocks, count=None, lr=False):
        """Row i: the dequantised MDCT coefficients, noise fill included, of blocks first[i] .. first[i] + n_blocks - 1 of file
        files[i] (the leading count[i] of them when `count` is given; zeros behind) - crops() stopped in front of the inverse
        transform (ulcx_decode_crops_spectra_dev).  The channels are the coded ones (mid / side for a pair) unless `lr`; a block's
        sub-blocks lie in coded order: ulc_amd.window_subblocks(BlockSize, wc) splits it.  No delay compensation.
        -> (coef [n][nChan][n_blocks][BlockSize] float32, wc int32 [n][n_blocks], bits int32 [n][n_blocks]) on the device, enqueued
        on torch's current stream.  `dec`: as for crops(); no stream state of it is read or changed."""
        import torch
        sfx, corpus = self._ready(dec)._view()
        n, files, first, want = self._rows(files, first, count)
        coef = torch.empty((n, self.C, n_blocks, self.BS), dtype=torch.float32, device=self.device)
        wc = torch.empty((n, n_blocks), dtype=torch.int32, device=self.device)
        bits = torch.empty((n, n_blocks), dtype=torch.int32, device=self.device)
        getattr(dec, f"decode_crops_spectra{sfx}_dev")(*corpus, n, files.data_ptr(), first.data_ptr(), _ptr(want), n_blocks, ulc_amd.SPECTRA_LR if lr else 0,
                                                       coef.data_ptr(), wc.data_ptr(), bits.data_ptr(),
                                                       stream=torch.cuda.current_stream(self.device).cuda_stream)
        return coef, wc, bits

    def distortion(self, dec, files, first, n_blocks, ref=None, ref_row=None, ref_first=None, count=None, n_seg=1, lr=False):
        """Row i: spectra()'s coefficients summed on chip against reference planes instead of written
        (ulcx_decode_crops_distortion_dev): per (row, channel, block, segment of BlockSize / n_seg coefficients) the binary64 sums
        {S, Y, E} = {reference energy, coded energy, error energy}, added in one fixed order (include/ulc_amd.h).  ref: float32
        [n_ref][nChan][n_ref_blocks][BlockSize] on the device, typically clip_spectra()'s planes (made with the same `lr`), or None:
        no reference, S = 0 and E = Y.  ref_row[i]: the reference row of crop row i (None: i); ref_first[i]: the reference block
        beside output block 0 (None: 0); a row or a block outside the reference counts as zeros.  n_seg: a power of two, 1 .. 64.
        -> (dist float64 [n][nChan][n_blocks][n_seg][3], wc int32 [n][n_blocks], bits int32 [n][n_blocks]) on the device, enqueued on
        torch's current stream; a contiguous `ref` is not copied.  `dec`: as for crops(); no stream state of it is read or changed."""
        import torch
        sfx, corpus = self._ready(dec)._view()
        n, files, first, want, row, rfirst = self._rows(files, first, count, ref_row, ref_first)
        n_ref = n_ref_blocks = 0
        if ref is not None:
            ref = torch.as_tensor(ref, dtype=torch.float32, device=self.device).contiguous()
            if ref.dim() != 4 or ref.shape[1] != self.C or ref.shape[3] != self.BS:
                raise UlcError(f"corpus: reference planes of shape {tuple(ref.shape)} for a corpus of {self.BS} x {self.C}")
            n_ref, n_ref_blocks = ref.shape[0], ref.shape[2]
        dist = torch.empty((n, self.C, n_blocks, n_seg, 3), dtype=torch.float64, device=self.device)
        wc = torch.empty((n, n_blocks), dtype=torch.int32, device=self.device)
        bits = torch.empty((n, n_blocks), dtype=torch.int32, device=self.device)
        getattr(dec, f"decode_crops_distortion{sfx}_dev")(*corpus, n, files.data_ptr(), first.data_ptr(), _ptr(want), n_blocks, _ptr(ref), n_ref, n_ref_blocks,
                                                          _ptr(row), _ptr(rfirst), int(n_seg), ulc_amd.SPECTRA_LR if lr else 0, dist.data_ptr(), wc.data_ptr(),
                                                          bits.data_ptr(), stream=torch.cuda.current_stream(self.device).cuda_stream)
        return dist, wc, bits


def rung_plan(dist_by_rung, blocks, target_db):
    """The plan CropCorpus.switch() takes, from the distortion of every rung of a ladder: dist_by_rung[r][clip][ch][k][seg][3] is
    CropCorpus.distortion() of file file_of(r, clip) from block 0 against the clip's clean planes (a tensor, or a sequence of
    one tensor per rung; CPU or device).  A block's SNR is 10 log10(sum S / sum E) over its channels and segments - E = 0: +inf;
    S = 0 with E > 0: -inf.  Block k of a clip takes the first rung, in the ladder's order, whose SNR reaches target_db, else the
    last rung; equal neighbours merge.  blocks[clip]: the blocks of the clip (the row's leading ones are planned).
    -> [[(rung, n_blocks), ...] per clip].  Pure tensor arithmetic in a fixed order - the same plan from the same bits on a CPU
    and on a device tensor; one transfer of the chosen rungs to the host."""
    import torch
    d = dist_by_rung if torch.is_tensor(dist_by_rung) else torch.stack(list(dist_by_rung))
    if d.dim() != 6 or d.shape[-1] != 3:
        raise UlcError(f"rung_plan: distortion of shape {tuple(d.shape)}, not [rung][clip][channel][block][segment][3]")
    if d.shape[4] & (d.shape[4] - 1):
        raise UlcError(f"rung_plan: {d.shape[4]} segments (a power of two, as the distortion calls give)")
    # a block's sums in ONE order on every device, so that a plan is a function of the distortion's bits: the segments up the
    # calls' own pairwise tree, then the channels in order; the target as a ratio, compared without a logarithm
    t = d.to(torch.float64)[..., (0, 2)]
    while t.shape[4] > 1:
        t = t[:, :, :, :, 0::2] + t[:, :, :, :, 1::2]
    t = t[:, :, :, :, 0]                                                        # [rung][clip][ch][block][2]
    tot = t[:, :, 0]
    for ch in range(1, t.shape[2]):
        tot = tot + t[:, :, ch]
    S, E = tot[..., 0], tot[..., 1]                                             # [rung][clip][block]
    ratio = 10.0 ** (float(target_db) / 10.0)                                   # SNR >= target_db  <=>  S >= ratio * E
    ok = (E == 0) | (S >= ratio * E)                                            # E = 0: +inf reaches; S = 0 with E > 0: -inf does not
    n_rungs = d.shape[0]
    first = torch.where(ok.any(dim=0), ok.to(torch.int8).argmax(dim=0), torch.full(ok.shape[1:], n_rungs - 1, dtype=torch.int64, device=d.device))
    first = first.cpu().numpy()
    blocks = np.asarray(torch.as_tensor(blocks).cpu() if torch.is_tensor(blocks) else blocks, np.int64).reshape(-1)
    if blocks.shape[0] != first.shape[0]:
        raise UlcError(f"rung_plan: {blocks.shape[0]} block counts for {first.shape[0]} clips")
    plan = []
    for clip in range(first.shape[0]):
        row = first[clip, :max(0, min(int(blocks[clip]), first.shape[1]))]
        cut = np.flatnonzero(np.diff(row)) + 1
        edges = np.concatenate([[0], cut, [len(row)]])
        plan.append([(int(row[a]), int(b - a)) for a, b in zip(edges[:-1], edges[1:]) if b > a])
    return plan
