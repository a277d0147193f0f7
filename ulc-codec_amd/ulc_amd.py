"""ctypes binding of libulc_amd.so (include/ulc_amd.h).  Plumbing only: no compute
happens here and there is no fallback — if the shared library or a GPU is missing the
constructors raise."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ULC_AMD_LIB: another build of the same library (A/B timing runs, tools/ab_all.sh); the default is the in-tree one
LIB_PATH = os.environ.get("ULC_AMD_LIB") or os.path.join(_HERE, "libulc_amd.so")

MODE_VBR, MODE_CBR, MODE_ABR = 0, 1, 2
_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)

N_BARK, MAX_SUB, BARK_EVENTS = 25, 4, 52
FRONT_PLAN_WORDS = 44            # include/ulc_amd.h: ULCX_FRONT_PLAN_WORDS
PLAN_FIELDS = ("bark_ring", "most_open", "use_gap_sums", "heap_in_lds", "ns_slots", "wc_pipe", "sel_pair")

MAX_RUNGS = 8                                              # ULCX_MAX_RUNGS
RUNG_AUTO = 1                                              # ULCX_RUNG_AUTO: Rung.reserved of the clips ladder calls
SPECTRA_LR = 1                                             # ULCX_SPECTRA_LR: flags of the spectra calls
SYNTH_WARM = 2                                             # ULCX_SYNTH_WARM: flags of the synth calls - plane 0 is the block in front

# one entry of a block index (include/ulc_amd.h, ulcx_index_entry): 8 bytes
INDEX_DTYPE = np.dtype([("ByteOffs", np.int32), ("RngState", np.uint32)])
# one segment of a splice (ulcx_segment): blocks First .. First + Count - 1 of source file File; 12 bytes
SEGMENT_DTYPE = np.dtype([("File", np.int32), ("First", np.int32), ("Count", np.int32)])


class FileHeader(C.Structure):
    """tools/ulc_Helper.h:10-20 (24 bytes)."""
    _fields_ = [("Magic", C.c_uint32), ("BlockSize", C.c_uint16), ("MaxBlockSize", C.c_uint16), ("nBlocks", C.c_uint32),
                ("RateHz", C.c_uint32), ("nChan", C.c_uint16), ("RateKbps", C.c_uint16), ("StreamOffs", C.c_uint32)]


class IndexFileHeader(C.Structure):
    """ulcx_index_file_header (include/ulc_amd.h): the 16-byte header of a `.ulx` sidecar."""
    _fields_ = [("Magic", C.c_uint32), ("BlockSize", C.c_uint16), ("nChan", C.c_uint16), ("nBlocks", C.c_uint32), ("PayloadBytes", C.c_uint32)]


class Rung(C.Structure):
    """ulcx_rung (include/ulc_amd.h): one rung of a ladder call, 24 bytes; rate NULL = the scalar setting."""
    _fields_ = [("mode", C.c_int32), ("param0", C.c_float), ("param1", C.c_float), ("reserved", C.c_int32), ("rate", C.c_void_p)]


# ---- The C ABI's signatures: export name -> (argtypes, restype).  Built without the library, so that
# tests/test_binding_signatures.py can hold every entry against include/ulc_amd.h; lib() applies it.
SIGNATURES = {}
PCM16_TWIN = {}                                            # device form -> its int16 twin (their names follow no one rule)
_vp, _int, _flt, _ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
_f64p, _u32p, _rungp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(Rung)
_DEVICE_PTR = {_f32p: _vp, _i32p: _vp, _u8p: _vp, _i64p: _vp, _f64p: _vp}


def _sig(names, argtypes, restype=C.c_int, table=None):
    for name in names.split():
        (SIGNATURES if table is None else table)[name] = (argtypes, restype)


def _dev(host):
    """Device form = the host form's arguments with every buffer a raw device pointer, then the stream."""
    return [_DEVICE_PTR.get(t, t) for t in host] + [_vp]


def _family(names, host, pcm16=False, table=None, twins=None):
    """A call family from its host form: names.format("host" / "dev" / "dev_pcm16"); an int16 twin shares its sibling's entry."""
    _sig(names.format("host"), host, table=table)
    _sig(names.format("dev") + (" " + names.format("dev_pcm16") if pcm16 else ""), _dev(host), table=table)
    if pcm16:
        (PCM16_TWIN if twins is None else twins)[names.format("dev")] = names.format("dev_pcm16")


# shared runs of arguments (the first of every list below is the object's handle unless the comment says otherwise)
_STRIDED = [_u8p, _ll, _i32p, _vp, _int, _i32p]            # payload, stride, payloadBytes, index, indexStride, indexBlocks
_RAGGED = [_u8p, _ll, _i64p, _vp, _ll, _i64p, _i32p]       # payload, total, payloadOffs, index, entries, indexOffs, indexBlocks
_CODED = [_u8p, _i32p, _i32p, _f32p]                       # out, bits, wc, cplx of the block-form encode calls
_PCM = [_f32p, _i32p]                                      # pcm, bits
_SPECTRA = [_int, _f32p, _i32p, _i32p]                     # flags, coef, wc, bits
_DIST = [_f32p, _int, _int, _i32p, _i32p, _int, _int, _f64p, _i32p, _i32p]   # ref, nRef, nRefBlocks, refRow, refFirst, nSeg, flags, dist, wc, bits
_TAP = [_int, _int, _f32p, _i32p, _f32p]                   # nBlocks, flags, coef, wc, cplx
_CLIPS_OUT = [_u8p, _ll, _i32p, _i32p, _vp, _int, _i32p]   # payload, stride, payloadBytes, maxBlock, index, indexStride, indexBlocks
_SPLICE_OUT = [_int, _i32p, _vp, _int] + _CLIPS_OUT + [_i32p]                # nOut, segOffs, seg, nSeg, the new corpus, segStart


def _rows(pos):
    return [_int, _i32p, pos, _i32p, _int]                 # n, file, first (int32) or start (int64), count or length, nBlocks or nSamples


# the drop-in ABI (the state structs, void * and int * are the caller's own types)
_sig("ULC_EncoderState_Init ULC_DecoderState_Init", [_vp])
_sig("ULC_EncoderState_Destroy ULC_DecoderState_Destroy", [_vp], None)
_sig("ULC_EncodeBlock_CBR ULC_EncodeBlock_VBR", [_vp, _f32p, _vp, _flt], _vp)
_sig("ULC_EncodeBlock_ABR", [_vp, _f32p, _vp, _flt, _flt], _vp)
_sig("ULC_DecodeBlock", [_vp, _f32p, _vp])
# the library, objects and their scalar queries
_sig("ulcx_last_error ulcx_build_rev", [], C.c_char_p)
_sig("ulcx_encoder_stage_name ulcx_decoder_stage_name", [_int], C.c_char_p)
_sig("ulcx_device_count", [])
_sig("ulcx_encoder_create", [C.POINTER(_vp), _int, _int, _int, _int, _int, _int])
_sig("ulcx_decoder_create", [C.POINTER(_vp), _int, _int, _int, _int, _int])
_sig("ulcx_encoder_reset ulcx_encoder_slot_bytes ulcx_encoder_last_rungs ulcx_encoder_last_fallbacks "
     "ulcx_encoder_last_xf_launches ulcx_decoder_reset", [_vp])
_sig("ulcx_encoder_destroy ulcx_decoder_destroy", [_vp], None)
_sig("ulcx_encoder_stream_state_bytes ulcx_decoder_stream_state_bytes", [_vp], C.c_size_t)
_sig("ulcx_encoder_set_timing ulcx_decoder_set_timing ulcx_encoder_debug_force_exact", [_vp, _int])
_sig("ulcx_encoder_stage_ms ulcx_decoder_stage_ms", [_vp, _f32p, _int])
_sig("ulcx_encoder_debug_fetch", [_vp, _int, _f32p, _f32p, _f32p, _u8p, _i32p])
_sig("ulcx_encoder_debug_writer_flags ulcx_encoder_debug_front_plan", [_vp, _int, _i32p])
_sig("ulcx_encoder_debug_writer_plan ulcx_encoder_debug_plan", [_vp, _i32p])
_sig("ulcx_decoder_last_cut", [_vp, _i32p, _i32p, _i32p])
# host arithmetic (no handle)
_sig("ulcx_debug_band_plan", [_int, _int, C.POINTER(C.c_int16), _i32p, _i32p])
_sig("ulcx_debug_band_events", [_int, _int, _u32p])
_sig("ulcx_dec_split_plan", [_int, _int, _int])
_sig("ulcx_dec_tail_plan ulcx_dec_range_tail_plan", [_int, _int, _int, _i32p])
_sig("ulcx_crop_blocks ulcx_clip_blocks", [_int, _int])
_sig("ulcx_window_subblocks", [_int, _int, _i32p])
_sig("ulcx_block_extent_bytes", [_vp, _int, _int, _int])
_sig("ulcx_index_check", [_vp, _int, _int, _ll])
_sig("ulcx_ulc_header_pack", [_u8p, C.POINTER(FileHeader)], None)
_sig("ulcx_ulc_header_parse", [C.POINTER(FileHeader), _u8p, C.c_size_t])
_sig("ulcx_ulc_rate_kbps", [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32])
_sig("ulcx_ulx_header_pack", [_u8p, C.POINTER(IndexFileHeader)], None)
_sig("ulcx_ulx_header_parse", [C.POINTER(IndexFileHeader), _u8p, C.c_size_t])
# the block forms: slots in, slots out
_family("ulcx_encode_{}", [_vp, _int, _flt, _flt, _f32p, _int] + _CODED, pcm16=True)
_family("ulcx_encode_{}_rates", [_vp, _f32p, _f32p, _int] + _CODED, pcm16=True)
_family("ulcx_encode_{}_ladder", [_vp, _rungp, _int, _f32p, _int] + _CODED, pcm16=True)
_family("ulcx_encode_{}_subset", [_vp, _i32p, _int, _int, _flt, _flt, _f32p, _f32p, _int] + _CODED, pcm16=True)
_family("ulcx_analyse_{}", [_vp, _f32p, _int, _i32p, _f32p], pcm16=True)
_sig("ulcx_analyse_dev_subset", _dev([_vp, _i32p, _int, _f32p, _int, _i32p, _f32p]))
_family("ulcx_decode_{}", [_vp, _u8p, _int, _int] + _PCM, pcm16=True)
_family("ulcx_decode_{}_subset", [_vp, _i32p, _int, _u8p, _int, _int] + _PCM, pcm16=True)
_sig("ulcx_encode_block1", [_vp, _int, _flt, _flt, _f32p, _u8p, _i32p, _f32p, _i32p, _f32p])
_sig("ulcx_decode_block1", [_vp, _u8p, _int, _f32p, _i32p, _i32p])
_sig("ulcx_decode_block1_rng", [_vp, _u8p, _int, _f32p, _i32p, _i32p, _u32p])
for _kind in ("encoder", "decoder"):                      # stream slots
    _family(f"ulcx_{_kind}_reset_streams_{{}}", [_vp, _i32p, _int])
    _family(f"ulcx_{_kind}_save_streams_{{}}", [_vp, _i32p, _int, _u8p])
    _family(f"ulcx_{_kind}_load_streams_{{}}", [_vp, _i32p, _int, _u8p])
# packed streams, their index, ranges
_sig("ulcx_pack_streams_dev", [_int, _int, _int, _int, _vp, _vp, _vp, _ll, _vp, _vp, _vp])
_family("ulcx_decode_packed_{}", [_vp, _u8p, _ll, _i32p, _int] + _PCM)
_family("ulcx_index_packed_{}", [_vp, _u8p, _ll, _i32p, _int, _vp, _i32p])
_family("ulcx_index_packed_rows_{}", [_vp, _int, _u8p, _ll, _i32p, _int, _vp, _i32p])
_family("ulcx_index_packed_ragged_{}", [_vp, _int] + _RAGGED)          # (indexBlocks is the output here)
_sig("ulcx_index_begin_dev", [_vp, _int, _vp, _int, _vp, _vp])
_family("ulcx_index_slots_{}", [_vp, _int, _u8p, _int, _i32p, _int, _vp, _int, _i32p])
_family("ulcx_decode_range_{}", [_vp] + _STRIDED + [_i32p, _int] + _PCM, pcm16=True)
_sig("ulcx_decoder_upload_payload", [_vp, _u8p, _ll, _i32p])
_sig("ulcx_decoder_index_resident", [_vp, _int, _i32p])
_sig("ulcx_decoder_set_resident_index", [_vp, _vp, _int, _i32p])
_sig("ulcx_decode_resident_host", [_vp, _int] + _PCM)
_sig("ulcx_decode_resident_range_host", [_vp, _i32p, _int] + _PCM)
# the families over a corpus, once per layout: handle, nFiles, the corpus, the rows, the family's tail
for _sfx, _view in (("", _STRIDED), ("_ragged", _RAGGED)):
    _family(f"ulcx_decode_crops{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i32p) + _PCM, pcm16=True)
    _family(f"ulcx_decode_crops_samples{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i64p) + _PCM, pcm16=True)
    _family(f"ulcx_decode_crops_spectra{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i32p) + _SPECTRA)
    _family(f"ulcx_decode_crops_distortion{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i32p) + _DIST)
    _family(f"ulcx_corpus_splice{_sfx}_{{}}", [_vp, _int] + _view + _SPLICE_OUT)
_family("ulcx_corpus_ragged_{}", [_int, _int] + _STRIDED + _RAGGED + [_i64p])     # device, nFiles, strided in, ragged out, need
_family("ulcx_synth_spectra_{}", [_vp, _int, _int, _int, _f32p, _i32p] + _PCM, pcm16=True)
# clips: encoder, decoder, n, the setting, pcm, len, nSamples, the corpus they write
_CLIPS = [_vp, _vp, _int, _int, _flt, _flt, _f32p, _f32p, _i32p, _int] + _CLIPS_OUT
_family("ulcx_encode_clips_{}", _CLIPS, pcm16=True)
_family("ulcx_encode_clips_spectra_{}", _CLIPS + _TAP, pcm16=True)
_family("ulcx_encode_clips_ladder_{}", [_vp, _vp, _int, _rungp, _int, _f32p, _i32p, _int] + _CLIPS_OUT + [_f32p], pcm16=True)
_family("ulcx_analyse_clips_{}", [_vp, _int, _f32p, _i32p, _int] + _TAP, pcm16=True)

EXPORTS = list(SIGNATURES)

# ---- The second table: the entries of the headers beside ulc_amd.h (include/ulc_amd_lowrate.h), built and applied as the first.
EXT_SIGNATURES = {}
EXT_PCM16_TWIN = {}
_sig("ulcx_lowrate_block", [_int, _int], table=EXT_SIGNATURES)
for _sfx, _view in (("", _STRIDED), ("_ragged", _RAGGED)):    # the sample-crop rows with lgD behind nSamples
    _family(f"ulcx_decode_crops_lowrate{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i64p) + [_int] + _PCM, pcm16=True,
            table=EXT_SIGNATURES, twins=EXT_PCM16_TWIN)
EXT_EXPORTS = list(EXT_SIGNATURES)

# ---- The third table: mid and side crops (include/ulc_amd_part.h), built and applied as the second.
PART_SIGNATURES = {}
PART_PCM16_TWIN = {}
PART_MID, PART_SIDE = 0, 1
_sig("ulcx_part_channels", [_int, _int], table=PART_SIGNATURES)
for _sfx, _view in (("", _STRIDED), ("_ragged", _RAGGED)):    # the low-rate rows with part behind lgD
    _family(f"ulcx_decode_crops_part{_sfx}_{{}}", [_vp, _int] + _view + _rows(_i64p) + [_int, _int] + _PCM, pcm16=True,
            table=PART_SIGNATURES, twins=PART_PCM16_TWIN)
PART_EXPORTS = list(PART_SIGNATURES)


def new_index(n_rows, index_stride):
    """An open index as ulcx_index_begin_dev leaves it: entry 0 = (0, 1234567), every other entry (-1, 0)."""
    index = np.zeros((n_rows, index_stride), INDEX_DTYPE)
    index["ByteOffs"][:, 1:] = -1
    index["RngState"][:, 0] = 1234567
    return index


def index_check(row, n_blocks, payload_bytes):
    """ulcx_index_check (host code, no GPU): True when `row` may be handed to a range call for a payload of payload_bytes."""
    row = np.ascontiguousarray(row, dtype=INDEX_DTYPE)
    return lib().ulcx_index_check(row.ctypes.data, int(n_blocks), row.shape[0], int(payload_bytes)) == 0


def ulx_pack(row, n_blocks, block_size, n_chan, payload_bytes):
    """Bytes of a `.ulx` sidecar: the 16-byte header and entries 0 .. n_blocks of `row`."""
    h = IndexFileHeader(0x31584C55, block_size, n_chan, int(n_blocks), int(payload_bytes))
    hb = (C.c_uint8 * 16)()
    lib().ulcx_ulx_header_pack(hb, C.byref(h))
    return bytes(hb) + np.ascontiguousarray(row[:int(n_blocks) + 1], dtype=INDEX_DTYPE).tobytes()


def ulx_parse(data):
    """-> (IndexFileHeader, entries [nBlocks + 1]) of a `.ulx` sidecar's bytes; raises UlcError on a short or foreign file."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h = IndexFileHeader()
    _call("ulcx_ulx_header_parse", C.byref(h), buf, len(data))
    body = data[16:16 + 8 * (h.nBlocks + 1)]
    if len(body) != 8 * (h.nBlocks + 1):
        raise UlcError(f"ulx: {h.nBlocks} blocks need {8 * (h.nBlocks + 1)} bytes of entries, the file has {len(data) - 16}")
    return h, np.frombuffer(body, INDEX_DTYPE).copy()


_lib = None
_bound = {}                                                # export name -> its function of lib(), resolved once


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `make -C ulc-codec_amd` (or __graft_entry__.build())")
        l = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in list(SIGNATURES.items()) + list(EXT_SIGNATURES.items()) + list(PART_SIGNATURES.items()):
            fn = getattr(l, name, None)                    # (an older build named by ULC_AMD_LIB for an A/B run may lack some)
            if fn is not None:
                fn.argtypes, fn.restype = argtypes, restype
        _lib = l
    return _lib


class UlcError(RuntimeError):
    pass


def _check(rc, what):
    if rc != 0:
        raise UlcError(f"{what} failed ({rc}): {lib().ulcx_last_error().decode()}")


def _bind(name):
    fn = _bound[name] = getattr(lib(), name)
    return fn


def _call(name, *args):
    """One call of an export that returns a status: _check() is told the name that was called."""
    _check((_bound.get(name) or _bind(name))(*args), name)


def _dev_call(name, pcm16, stream, *args):
    """A device form: `name` or, with pcm16, its int16 twin; the stream goes last (0: the null stream).  (Not through _call():
    bench.py's timed loop comes through here, and a second frame per call is all the cost there is to save.)"""
    if pcm16:
        name = next(t[name] for t in (PCM16_TWIN, EXT_PCM16_TWIN, PART_PCM16_TWIN) if name in t)
    _check((_bound.get(name) or _bind(name))(*args, stream or None), name)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _payload_view(ragged, payload, sizes):
    """The payloads of F files as the host forms take them -> (F, the C argument run).  Strided: payload uint8 [F][stride],
    sizes = payload_bytes [F].  Ragged: payload uint8 [total], sizes = payload_offs int64 [F + 1]."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    if ragged:
        payload = payload.reshape(-1)
        poffs = np.ascontiguousarray(sizes, dtype=np.int64)
        assert poffs.ndim == 1
        return poffs.shape[0] - 1, (_p(payload, _u8p), payload.size, _p(poffs, _i64p))
    nbytes = np.ascontiguousarray(sizes, dtype=np.int32)
    F, stride = payload.shape
    assert nbytes.shape == (F,)
    return F, (_p(payload, _u8p), stride, _p(nbytes, _i32p))


def _corpus_view(ragged, payload, sizes, index, index_offs, index_blocks):
    """A corpus as the host forms take it -> (F, the C argument run): _payload_view(), then index [F][index_stride] (ragged:
    [entries] behind index_offs int64 [F + 1]) and index_blocks [F].  The run's pointers keep their arrays alive."""
    F, src = _payload_view(ragged, payload, sizes)
    index = np.ascontiguousarray(index, dtype=INDEX_DTYPE)
    blocks = np.ascontiguousarray(index_blocks, dtype=np.int32)
    assert blocks.shape == (F,)
    if ragged:
        index = index.reshape(-1)
        ioffs = np.ascontiguousarray(index_offs, dtype=np.int64)
        assert ioffs.shape == (F + 1,)
        return F, src + (_p(index, _vp), index.size, _p(ioffs, _i64p), _p(blocks, _i32p))
    assert index.shape[0] == F
    return F, src + (_p(index, _vp), index.shape[1], _p(blocks, _i32p))


def _row_view(files, pos, pos_dtype, want):
    """The rows of a crop call -> (n, the C argument run n, files, positions, counts): files [n], pos [n] of pos_dtype (int32
    first blocks, int64 start samples), want [n] or None."""
    files = np.ascontiguousarray(files, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=pos_dtype)
    want = None if want is None else np.ascontiguousarray(want, dtype=np.int32)
    n = files.shape[0]
    assert pos.shape == (n,) and (want is None or want.shape == (n,))
    return n, (n, _p(files, _i32p), _p(pos, _i64p if pos_dtype is np.int64 else _i32p), _p(want, _i32p))


def crop_blocks(block_size, n_samples):
    """Blocks a crop of n_samples samples touches at the worst start (ulcx_crop_blocks): a sample-crop call's d_bits row, and
    what max_blocks - 1 of its decoder must reach."""
    return int(lib().ulcx_crop_blocks(int(block_size), int(n_samples)))


def lowrate_block(block_size, lowrate):
    """BlockSize of the reduced stream of a low-rate crop (ulcx_lowrate_block): block_size >> lowrate for lowrate 0 .. 3 when that is
    a legal BlockSize, else 0."""
    return int(lib().ulcx_lowrate_block(int(block_size), int(lowrate)))


def part_channels(n_chan, part):
    """Planes per row of a mid / side crop (ulcx_part_channels): (n_chan + 1 - part) // 2 for part PART_MID / PART_SIDE, else 0."""
    return int(lib().ulcx_part_channels(int(n_chan), int(part)))


def window_subblocks(block_size, wc):
    """Sizes, in coded order, of the sub-blocks of a block with window code `wc` (ulcx_window_subblocks; host arithmetic): how the
    block_size coefficients of a spectra call's block split into shorter spectra.  () for a code no block can carry - 0, a block
    that is not live, among them - or a bad block size."""
    sizes = (C.c_int32 * 4)()
    n = lib().ulcx_window_subblocks(int(block_size), int(wc), sizes)
    return tuple(int(sizes[j]) for j in range(n))


def clip_blocks(block_size, n_samples):
    """Blocks of a clip of n_samples samples (ulcx_clip_blocks): what the reference tool writes for a file of that length,
    (n_samples + block_size - 1) // block_size + 2; 0 for an empty clip or a bad block size."""
    return int(lib().ulcx_clip_blocks(int(block_size), int(n_samples)))


def corpus_ragged_dev(n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, d_out_payload, payload_cap, d_payload_offs,
                      d_out_index, index_cap, d_index_offs, d_out_index_blocks, d_need, stream=0, device=0):
    """ulcx_corpus_ragged_dev: a strided corpus on the device into the ragged layout (raw device pointers; asynchronous on
    `stream`).  d_payload_offs / d_index_offs int64 [n_files + 1], d_out_index_blocks int32 [n_files], d_need int64 [2]: the bytes
    and entries the whole corpus needs.  Files behind the first one that does not fit the capacities come out empty."""
    _dev_call("ulcx_corpus_ragged_dev", False, stream, int(device), int(n_files), d_payload, int(stride), d_payload_bytes, d_index, int(index_stride),
              d_index_blocks, d_out_payload, int(payload_cap), d_payload_offs, d_out_index, int(index_cap), d_index_offs, d_out_index_blocks, d_need)


def corpus_ragged(payload, payload_bytes, index, index_blocks, payload_cap=None, index_cap=None, device=0):
    """Host form (ulcx_corpus_ragged_host): payload uint8 [F][stride], payload_bytes [F], index [F][index_stride], index_blocks [F]
    -> dict(payload uint8 [payload_cap], payload_offs int64 [F + 1], index [index_cap], index_offs int64 [F + 1], index_blocks [F],
    need int64 [2]).  Without capacities: what the whole corpus needs (host arithmetic)."""
    F, src = _corpus_view(False, payload, payload_bytes, index, None, index_blocks)
    stride, index_stride = src[1], src[4]
    if payload_cap is None:
        payload_cap = int(np.clip(np.asarray(payload_bytes, dtype=np.int32).astype(np.int64), 0, stride).sum())
    if index_cap is None:
        index_cap = int((np.clip(np.asarray(index_blocks, dtype=np.int32).astype(np.int64), 0, index_stride - 1) + 1).sum())
    r = dict(payload=np.zeros(max(1, payload_cap), np.uint8), payload_offs=np.zeros(F + 1, np.int64), index=np.zeros(max(1, index_cap), INDEX_DTYPE),
             index_offs=np.zeros(F + 1, np.int64), index_blocks=np.zeros(F, np.int32), need=np.zeros(2, np.int64))
    _call("ulcx_corpus_ragged_host", int(device), F, *src, _p(r["payload"], _u8p), int(payload_cap), _p(r["payload_offs"], _i64p), r["index"].ctypes.data,
          int(index_cap), _p(r["index_offs"], _i64p), _p(r["index_blocks"], _i32p), _p(r["need"], _i64p))
    return r


def build_rev():
    """Revision of the sources the loaded library was built from (sha1 prefix, ulc-codec_amd/Makefile)."""
    return lib().ulcx_build_rev().decode()


class _StreamSlots:
    """Stream slots (include/ulc_amd.h): per-stream reset, save / load of single streams' state.  `slots` is a list of
    slots of the object (host forms: no duplicate, every entry in 0 .. B-1, checked before any device work); records are
    uint8 [n][state_bytes].  The *_dev forms take raw device pointers (ints / .data_ptr()) and are asynchronous on `stream`."""
    _kind = None

    def _name(self, what):
        return f"ulcx_{self._kind}_{what}"

    @staticmethod
    def _slots(slots):
        s = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        return s, _p(s, _i32p)

    @property
    def state_bytes(self):
        return int(getattr(lib(), self._name("stream_state_bytes"))(self.h))

    def reset_streams(self, slots):
        s, sp = self._slots(slots)
        _call(self._name("reset_streams_host"), self.h, sp, s.size)

    def save_streams(self, slots):
        s, sp = self._slots(slots)
        state = np.zeros((s.size, self.state_bytes), np.uint8)
        _call(self._name("save_streams_host"), self.h, sp, s.size, _p(state, _u8p))
        return state

    def load_streams(self, slots, state):
        s, sp = self._slots(slots)
        state = np.ascontiguousarray(state, dtype=np.uint8)
        assert state.size == s.size * self.state_bytes
        _call(self._name("load_streams_host"), self.h, sp, s.size, _p(state, _u8p))

    def reset_streams_dev(self, d_slots, n, stream=0):
        _dev_call(self._name("reset_streams_dev"), False, stream, self.h, d_slots, n)

    def save_streams_dev(self, d_slots, n, d_state, stream=0):
        _dev_call(self._name("save_streams_dev"), False, stream, self.h, d_slots, n, d_state)

    def load_streams_dev(self, d_slots, n, d_state, stream=0):
        _dev_call(self._name("load_streams_dev"), False, stream, self.h, d_slots, n, d_state)


def band_plan(block_size, rate_hz):
    """The Bark band tables an encoder of (block_size, rate_hz) is created with, host arithmetic only (no device, no object):
    edges int16 [noise|psycho][MAX_SUB][beg|end][N_BARK], the most bands open at one line of the full-size tables, and the snapshot
    ring ulcx_encoder_create derives from them (0: the lane-per-subblock kernels for every block).  Test hook."""
    edges = np.zeros((2, MAX_SUB, 2, N_BARK), np.int16)
    most, ring = np.zeros(1, np.int32), np.zeros(1, np.int32)
    _call("ulcx_debug_band_plan", int(block_size), int(rate_hz), _p(edges, C.POINTER(C.c_int16)), _p(most, _i32p), _p(ring, _i32p))
    return edges, int(most[0]), int(ring[0])


def band_events(block_size, rate_hz):
    """The band-edge lists k_bark_uniform walks: uint32 [noise|psycho][MAX_SUB][BARK_EVENTS] words line | kind << 16 | band << 24
    (kind 0: lower edge, 1: upper edge, 2: end of the subblock, 3: padding).  Test hook."""
    ev = np.zeros((2, MAX_SUB, BARK_EVENTS), np.uint32)
    _call("ulcx_debug_band_events", int(block_size), int(rate_hz), _p(ev, _u32p))
    return ev


class BatchEncoder(_StreamSlots):
    """B independent streams; encode(pcm[B][K*BS][C]) -> (bytes[B][K][slot], bits[B][K], wc[B][K], cplx[B][K])."""
    _kind = "encoder"

    def __init__(self, n_streams, n_chan, block_size, rate_hz, max_blocks, device=0):
        self.B, self.C, self.BS, self.rate, self.maxK = n_streams, n_chan, block_size, rate_hz, max_blocks
        self.h = C.c_void_p()
        _call("ulcx_encoder_create", C.byref(self.h), device, n_streams, n_chan, block_size, rate_hz, max_blocks)
        self.slot = lib().ulcx_encoder_slot_bytes(self.h)
        self.lastK = 0

    def close(self):
        if self.h:
            lib().ulcx_encoder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _call("ulcx_encoder_reset", self.h)

    def _blocks_in(self, pcm, n, lead=()):
        """The block forms' input and outputs: pcm float32 [n][K * BS][C] -> (pcm, K, and zeroed out uint8 lead + [n][K][slot],
        bits lead + [n][K], wc [n][K], cplx [n][K])."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        assert pcm.shape[0] == n and pcm.shape[-1] == self.C
        K = pcm.shape[1] // self.BS
        assert pcm.shape[1] == K * self.BS
        return (pcm, K, np.zeros(lead + (n, K, self.slot), np.uint8), np.zeros(lead + (n, K), np.int32), np.zeros((n, K), np.int32),
                np.zeros((n, K), np.float32))

    @staticmethod
    def _table(t, n):
        t = np.ascontiguousarray(t, dtype=np.float32)
        assert t.shape == (n, 2)
        return t

    def _host_table(self, n):
        """table_ptr of _rungs() for host tables float32 [n][2]; the closure keeps them alive, so hold it over the call."""
        tables = []

        def host_table(t):
            tables.append(self._table(t, n))
            return tables[-1].ctypes.data
        return host_table

    def encode(self, pcm, mode=MODE_VBR, p0=50.0, p1=0.0):
        pcm, K, out, bits, wc, cplx = self._blocks_in(pcm, self.B)
        _call("ulcx_encode_host", self.h, mode, p0, p1, _p(pcm, _f32p), K, _p(out, _u8p), _p(bits, _i32p), _p(wc, _i32p), _p(cplx, _f32p))
        self.lastK = K
        return out, bits, wc, cplx

    def encode_rates(self, pcm, rates):
        """As encode(), with a setting per stream: rates is float32 [B][2] = {RateKbps, AvgComplexity} per stream in the
        reference tool's convention (RateKbps < 0: VBR at quality -RateKbps; else AvgComplexity > 0: ABR; else CBR).
        Invalid entries (non-finite, RateKbps == 0, AvgComplexity < 0) raise before any device work."""
        pcm, K, out, bits, wc, cplx = self._blocks_in(pcm, self.B)
        rates = self._table(rates, self.B)
        _call("ulcx_encode_host_rates", self.h, _p(rates, _f32p), _p(pcm, _f32p), K, _p(out, _u8p), _p(bits, _i32p), _p(wc, _i32p), _p(cplx, _f32p))
        self.lastK = K
        return out, bits, wc, cplx

    def encode_dev_rates(self, d_rates, d_pcm, n_blocks, d_out, d_bits, d_wc=0, d_cplx=0, stream=0, pcm16=False):
        """Device-pointer path with a per-stream table: d_rates points to float32 [B][2] on the device (read by the call's
        kernels, so it may be rewritten between calls on the same stream); pcm16=True takes int16 samples."""
        _dev_call("ulcx_encode_dev_rates", pcm16, stream, self.h, d_rates, d_pcm, n_blocks, d_out, d_bits, d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    @staticmethod
    def _rungs(rungs, table_ptr):
        """ctypes array of ulcx_rung from a list whose entries are (mode, p0[, p1]) or a per-stream table; table_ptr(t) gives
        the table's address.  The clips ladder calls also take ("auto", kbps) and ("auto_table", table): ULCX_RUNG_AUTO on a
        scalar ABR rung or on a table rung.  No limit on the count here: the library checks it."""
        arr = (Rung * max(len(rungs), 1))()
        for r, g in enumerate(rungs):
            if isinstance(g, tuple) and isinstance(g[0], str):
                if g[0] not in ("auto", "auto_table"):
                    raise UlcError(f"rung {r}: {g[0]!r} (a mode number, 'auto' or 'auto_table')")
                arr[r].reserved = RUNG_AUTO
                if g[0] == "auto":
                    arr[r].mode, arr[r].param0 = MODE_ABR, float(g[1])
                else:
                    arr[r].rate = table_ptr(g[1])
            elif isinstance(g, tuple):
                arr[r].mode, arr[r].param0, arr[r].param1 = int(g[0]), float(g[1]), float(g[2]) if len(g) > 2 else 0.0
            else:
                arr[r].rate = table_ptr(g)
        return arr

    def encode_ladder(self, pcm, rungs):
        """One call, several rate settings: each rung is a tuple (mode, p0[, p1]) for the whole batch or a float32 array
        [B][2] = {RateKbps, AvgComplexity} per stream (as encode_rates takes it).  Returns out[R][B][K][slot], bits[R][B][K],
        wc[B][K], cplx[B][K]; the streams' state advances once."""
        R = len(rungs)
        pcm, K, out, bits, wc, cplx = self._blocks_in(pcm, self.B, lead=(max(R, 1),))
        host_table = self._host_table(self.B)
        _call("ulcx_encode_host_ladder", self.h, self._rungs(rungs, host_table), R, _p(pcm, _f32p), K, _p(out, _u8p), _p(bits, _i32p), _p(wc, _i32p),
              _p(cplx, _f32p))
        self.lastK = K
        return out, bits, wc, cplx

    def encode_dev_ladder(self, rungs, d_pcm, n_blocks, d_out, d_bits, d_wc=0, d_cplx=0, stream=0, pcm16=False):
        """Device-pointer ladder call, asynchronous on `stream`: rungs as in encode_ladder, a table rung being the device
        address (int / .data_ptr()) of float32 [B][2]; d_out [R][B][K][slot], d_bits [R][B][K]; pcm16=True takes int16 samples."""
        _dev_call("ulcx_encode_dev_ladder", pcm16, stream, self.h, self._rungs(rungs, int), len(rungs), d_pcm, n_blocks, d_out, d_bits, d_wc or None,
                  d_cplx or None)
        self.lastK = n_blocks

    def last_rungs(self):
        """Rungs of the last encode call (1 for a plain or per-stream-rates call, 0 after an analysis call)."""
        return int(lib().ulcx_encoder_last_rungs(self.h))

    def encode_dev(self, d_pcm, n_blocks, d_out, d_bits, d_wc=0, d_cplx=0, mode=MODE_VBR, p0=50.0, p1=0.0, stream=0):
        """Device-pointer path (ints / .data_ptr()); asynchronous on `stream`."""
        _dev_call("ulcx_encode_dev", False, stream, self.h, mode, p0, p1, d_pcm, n_blocks, d_out, d_bits, d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    def encode_dev_pcm16(self, d_pcm16, n_blocks, d_out, d_bits, d_wc=0, d_cplx=0, mode=MODE_VBR, p0=50.0, p1=0.0, stream=0):
        """PCM16 ingest: d_pcm16 is a device pointer to int16 [B][K][BS][C]; converted on load as tools/WavIO_Helper.c:49-55."""
        _dev_call("ulcx_encode_dev", True, stream, self.h, mode, p0, p1, d_pcm16, n_blocks, d_out, d_bits, d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    def analyse(self, pcm):
        """Analysis only (no selection, no writer): pcm[B][K*BS][C] -> (wc[B][K], cplx[B][K]), the WindowCtrl and
        BlockComplexity encode() returns for the same input; the streams' state advances as encode() advances it."""
        pcm, K, _, _, wc, cplx = self._blocks_in(pcm, self.B)
        _call("ulcx_analyse_host", self.h, _p(pcm, _f32p), K, _p(wc, _i32p), _p(cplx, _f32p))
        self.lastK = K
        return wc, cplx

    def analyse_dev(self, d_pcm, n_blocks, d_wc=0, d_cplx=0, stream=0, pcm16=False):
        """Device-pointer analysis call, asynchronous on `stream`; at least one of d_wc / d_cplx; pcm16=True takes int16 samples."""
        _dev_call("ulcx_analyse_dev", pcm16, stream, self.h, d_pcm, n_blocks, d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    def encode_subset(self, slots, pcm, mode=MODE_VBR, p0=50.0, p1=0.0, rates=None):
        """As encode() for the listed slots only: pcm [n][K*BS][C], row i for slot slots[i]; only those slots' state
        advances.  rates: float32 [n][2] per row as encode_rates takes it (mode / p0 / p1 are then unused)."""
        s, sp = self._slots(slots)
        n = s.size
        pcm, K, out, bits, wc, cplx = self._blocks_in(pcm, n)
        if rates is not None:
            rates = self._table(rates, n)
        _call("ulcx_encode_host_subset", self.h, sp, n, mode, p0, p1, _p(rates, _f32p), _p(pcm, _f32p), K, _p(out, _u8p), _p(bits, _i32p),
              _p(wc, _i32p), _p(cplx, _f32p))
        self.lastK = K
        return out, bits, wc, cplx

    def encode_subset_dev(self, d_slots, n, d_pcm, n_blocks, d_out, d_bits, d_wc=0, d_cplx=0, mode=MODE_VBR, p0=50.0, p1=0.0, d_rates=0,
                          stream=0, pcm16=False):
        """Device-pointer subset call, asynchronous on `stream`: d_slots int32 [n] on the device, every buffer [n][n_blocks]...;
        d_rates: device table [n] (0: the scalar setting); pcm16=True takes int16 samples."""
        _dev_call("ulcx_encode_dev_subset", pcm16, stream, self.h, d_slots, n, mode, p0, p1, d_rates or None, d_pcm, n_blocks, d_out, d_bits,
                  d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    def _clips_in(self, wave, lengths, rates=None):
        """The clips forms' input: wave float32 [n][C][T], lengths [n] or None, rates float32 [n][2] or None
        -> (n, T, the C pointers of rates, wave and lengths, NULL for a None)."""
        wave = np.ascontiguousarray(wave, dtype=np.float32)
        n, ch, T = wave.shape
        assert ch == self.C
        want = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
        assert want is None or want.shape == (n,)
        if rates is not None:
            rates = self._table(rates, n)
        return n, T, _p(rates, _f32p), _p(wave, _f32p), _p(want, _i32p)

    def _corpus_out(self, n, T, payload_stride, index_stride, lead=()):
        """The corpus a clips form writes, zeroed, lead + [n] files at the default strides (they hold every file in full) unless given
        -> (blocks of T samples, (payload, payload_bytes, max_block, index, index_blocks), their C argument run)."""
        nb = clip_blocks(self.BS, T)
        payload_stride = payload_stride or self.slot * nb
        index_stride = index_stride or nb + 1
        payload = np.zeros(lead + (n, payload_stride), np.uint8)
        nbytes, maxb, count = (np.zeros(lead + (n,), np.int32) for _ in range(3))
        index = np.zeros(lead + (n, index_stride), INDEX_DTYPE)
        return nb, (payload, nbytes, maxb, index, count), (_p(payload, _u8p), payload_stride, _p(nbytes, _i32p), _p(maxb, _i32p), index.ctypes.data,
                                                           index_stride, _p(count, _i32p))

    def _tap_out(self, n, depth, flags):
        """The planes of a tap, zeroed -> ((coef [n][C][depth][BS], wc [n][depth], cplx [n][depth]), their C argument run)."""
        coef = np.zeros((n, self.C, max(depth, 0), self.BS), np.float32)
        wc = np.zeros((n, max(depth, 0)), np.int32)
        cplx = np.zeros((n, max(depth, 0)), np.float32)
        return (coef, wc, cplx), (depth, flags, _p(coef, _f32p), _p(wc, _i32p), _p(cplx, _f32p))

    def encode_clips_dev(self, dec, n, d_pcm, d_len, n_samples, d_payload, payload_stride, d_payload_bytes, d_index, index_stride, d_index_blocks,
                         d_max_block=0, mode=MODE_VBR, p0=50.0, p1=0.0, d_rates=0, stream=0, pcm16=False):
        """Clips into a resident corpus (ulcx_encode_clips_dev), asynchronous on `stream`: d_pcm [n][C][n_samples] (int16 with
        pcm16), d_len int32 [n] or 0 (every row n_samples long), each row encoded from a fresh state under the scalar setting or
        d_rates [n]; d_payload [n][payload_stride], d_payload_bytes [n], d_index [n][index_stride], d_index_blocks [n].  `dec`: a
        BatchDecoder of this geometry (tables for the index).  No slot of the encoder is read or changed."""
        _dev_call("ulcx_encode_clips_dev", pcm16, stream, self.h, dec.h, n, mode, p0, p1, d_rates or None, d_pcm, d_len or None, n_samples, d_payload,
                  payload_stride, d_payload_bytes, d_max_block or None, d_index, index_stride, d_index_blocks)

    def encode_clips(self, dec, wave, lengths=None, mode=MODE_VBR, p0=50.0, p1=0.0, rates=None, payload_stride=None, index_stride=None):
        """Host form (ulcx_encode_clips_host): wave float32 [n][C][T], lengths [n] or None, rates float32 [n][2] or None
        -> (payload uint8 [n][payload_stride], payload_bytes [n], max_block [n], index [n][index_stride], index_blocks [n]).
        The default strides hold every row in full."""
        n, T, rates, wave, want = self._clips_in(wave, lengths, rates)
        _, corpus, out = self._corpus_out(n, T, payload_stride, index_stride)
        _call("ulcx_encode_clips_host", self.h, dec.h, n, mode, p0, p1, rates, wave, want, T, *out)
        return corpus

    def encode_clips_ladder_dev(self, dec, n, rungs, d_pcm, d_len, n_samples, d_payload, payload_stride, d_payload_bytes, d_index, index_stride, d_index_blocks,
                                d_max_block=0, d_avg=0, stream=0, pcm16=False):
        """encode_clips_dev() under several rate settings in one call (ulcx_encode_clips_ladder_dev): rungs as encode_dev_ladder
        takes them - (mode, p0[, p1]) or the device address of a float32 [n][2] table - and ("auto", kbps) / ("auto_table", table address):
        two-pass ABR at the clip's own average complexity.  The outputs hold R * n files, file r * n + i = clip i under rung r;
        d_avg float32 [n] (optional) receives the averages when a rung is "auto"."""
        _dev_call("ulcx_encode_clips_ladder_dev", pcm16, stream, self.h, dec.h, n, self._rungs(rungs, int), len(rungs), d_pcm, d_len or None, n_samples,
                  d_payload, payload_stride, d_payload_bytes, d_max_block or None, d_index, index_stride, d_index_blocks, d_avg or None)

    def encode_clips_ladder(self, dec, wave, lengths=None, rungs=((MODE_VBR, 50.0),), payload_stride=None, index_stride=None):
        """Host form (ulcx_encode_clips_ladder_host): wave float32 [n][C][T], lengths [n] or None; a rung is (mode, p0[, p1]), a
        float32 [n][2] table, ("auto", kbps) or ("auto_table", table)
        -> (payload uint8 [R][n][payload_stride], payload_bytes [R][n], max_block [R][n], index [R][n][index_stride], index_blocks [R][n],
            avg float32 [n]: the clips' average complexities, zeros without an "auto" rung).  The default strides hold every file in full."""
        n, T, _, wave, want = self._clips_in(wave, lengths)
        host_table = self._host_table(n)
        arr = self._rungs(rungs, host_table)
        R = len(rungs)
        _, corpus, out = self._corpus_out(n, T, payload_stride, index_stride, lead=(max(R, 1),))
        avg = np.zeros(n, np.float32)
        _call("ulcx_encode_clips_ladder_host", self.h, dec.h, n, arr, R, wave, want, T, *out, _p(avg, _f32p))
        return (*corpus, avg)

    def encode_clips_spectra_dev(self, dec, n, d_pcm, d_len, n_samples, d_payload, payload_stride, d_payload_bytes, d_index, index_stride, d_index_blocks,
                                 n_blocks, d_coef, d_wc=0, d_cplx=0, flags=0, d_max_block=0, mode=MODE_VBR, p0=50.0, p1=0.0, d_rates=0, stream=0,
                                 pcm16=False):
        """encode_clips_dev() with the tap (ulcx_encode_clips_spectra_dev): the same corpus, and the encoder's own MDCT coefficients
        of the same blocks in d_coef float32 [n][C][n_blocks][BS], their window codes in d_wc int32 [n][n_blocks] and block
        complexities in d_cplx float32 [n][n_blocks] (0: not wanted).  flags: 0, or SPECTRA_LR."""
        _dev_call("ulcx_encode_clips_spectra_dev", pcm16, stream, self.h, dec.h, n, mode, p0, p1, d_rates or None, d_pcm, d_len or None, n_samples,
                  d_payload, payload_stride, d_payload_bytes, d_max_block or None, d_index, index_stride, d_index_blocks, n_blocks, flags,
                  d_coef or None, d_wc or None, d_cplx or None)

    def encode_clips_spectra(self, dec, wave, lengths=None, n_blocks=None, flags=0, mode=MODE_VBR, p0=50.0, p1=0.0, rates=None,
                             payload_stride=None, index_stride=None):
        """Host form (ulcx_encode_clips_spectra_host): encode_clips()'s arguments and results, followed by
        (coef float32 [n][C][n_blocks][BS], wc int32 [n][n_blocks], cplx float32 [n][n_blocks]); n_blocks None: every row in full."""
        n, T, rates, wave, want = self._clips_in(wave, lengths, rates)
        nb, corpus, out = self._corpus_out(n, T, payload_stride, index_stride)
        planes, tap = self._tap_out(n, nb if n_blocks is None else int(n_blocks), flags)
        _call("ulcx_encode_clips_spectra_host", self.h, dec.h, n, mode, p0, p1, rates, wave, want, T, *out, *tap)
        return (*corpus, *planes)

    def analyse_clips_dev(self, n, d_pcm, d_len, n_samples, n_blocks, d_coef, d_wc=0, d_cplx=0, flags=0, stream=0, pcm16=False):
        """The encoder's MDCT coefficients of clips without encoding them (ulcx_analyse_clips_dev), asynchronous on `stream`:
        d_pcm [n][C][n_samples] (int16 with pcm16), d_len int32 [n] or 0 -> d_coef float32 [n][C][n_blocks][BS], d_wc int32
        [n][n_blocks], d_cplx float32 [n][n_blocks] (0: not wanted).  No slot of the encoder is read or changed."""
        _dev_call("ulcx_analyse_clips_dev", pcm16, stream, self.h, n, d_pcm, d_len or None, n_samples, n_blocks, flags, d_coef or None, d_wc or None,
                  d_cplx or None)

    def analyse_clips(self, wave, lengths=None, n_blocks=None, flags=0):
        """Host form (ulcx_analyse_clips_host): wave float32 [n][C][T], lengths [n] or None
        -> (coef float32 [n][C][n_blocks][BS], wc int32 [n][n_blocks], cplx float32 [n][n_blocks]); n_blocks None: every row in full."""
        n, T, _, wave, want = self._clips_in(wave, lengths)
        planes, tap = self._tap_out(n, clip_blocks(self.BS, T) if n_blocks is None else int(n_blocks), flags)
        _call("ulcx_analyse_clips_host", self.h, n, wave, want, T, *tap)
        return planes

    def analyse_subset_dev(self, d_slots, n, d_pcm, n_blocks, d_wc=0, d_cplx=0, stream=0):
        _dev_call("ulcx_analyse_dev_subset", False, stream, self.h, d_slots, n, d_pcm, n_blocks, d_wc or None, d_cplx or None)
        self.lastK = n_blocks

    def debug_fetch(self, K=None, parts=("coef", "noise", "keys", "keep", "nout")):
        """The taps of the last call; `parts` names the ones to fetch (the others are not copied and come back as None)."""
        K = K or self.lastK
        n = self.C * self.BS
        shapes = dict(coef=((self.B, K, n), np.float32), noise=((self.B, K, n), np.float32), keys=((self.B, K, n), np.float32),
                      keep=((self.B, K, n), np.uint8), nout=((self.B, K), np.int32))
        unknown = set(parts) - set(shapes)
        if unknown:
            raise ValueError(f"unknown taps: {sorted(unknown)}")
        r = {k: (np.zeros(*shapes[k]) if k in parts else None) for k in shapes}
        _call("ulcx_encoder_debug_fetch", self.h, K, _p(r["coef"], _f32p), _p(r["noise"], _f32p), _p(r["keys"], _f32p), _p(r["keep"], _u8p),
              _p(r["nout"], _i32p))
        return r

    def last_fallbacks(self):
        return lib().ulcx_encoder_last_fallbacks(self.h)

    def writer_flags(self, K=None):
        """int32 [B][K]: the wave writer's tier of every block of the last encode call (bit 0: left the small-capacity launch,
        bit 1: left to the serial kernel, bit 2: packed by the wave writer itself).  Test hook."""
        K = K or self.lastK
        flags = np.zeros((self.B, K), np.int32)
        _call("ulcx_encoder_debug_writer_flags", self.h, K, _p(flags, _i32p))
        return flags

    def writer_plan(self):
        """The wave writer's capacity tiers of this object: dict small / medium / full -> (kept, zones, nybbles), have_mid,
        have_full.  Test hook."""
        p = np.zeros(11, np.int32)
        _call("ulcx_encoder_debug_writer_plan", self.h, _p(p, _i32p))
        return dict(small=tuple(int(v) for v in p[0:3]), medium=tuple(int(v) for v in p[3:6]), full=tuple(int(v) for v in p[6:9]),
                    have_mid=bool(p[9]), have_full=bool(p[10]))

    def plan(self):
        """What create decided for this object: bark_ring (0, 4 or 8), most_open, use_gap_sums, heap_in_lds, ns_slots, wc_pipe,
        sel_pair.  Test hook."""
        p = np.zeros(len(PLAN_FIELDS), np.int32)
        _call("ulcx_encoder_debug_plan", self.h, _p(p, _i32p))
        return {k: int(v) for k, v in zip(PLAN_FIELDS, p)}

    def front_plan(self, n_blocks):
        """How the front half of a call of n_blocks would be cut on this object: (transform cuts, window-control step
        boundaries), each a tuple that runs from 0 to n_blocks.  Test hook."""
        p = np.zeros(FRONT_PLAN_WORDS, np.int32)
        _call("ulcx_encoder_debug_front_plan", self.h, int(n_blocks), _p(p, _i32p))
        n_ch, n_w = int(p[0]), int(p[1])
        return tuple(int(v) for v in p[2:3 + n_ch]), tuple(int(v) for v in p[3 + n_ch:4 + n_ch + n_w])

    def force_exact(self, every):
        _call("ulcx_encoder_debug_force_exact", self.h, int(every))

    def xf_launches(self):
        return int(lib().ulcx_encoder_last_xf_launches(self.h))

    def set_timing(self, on):
        _call("ulcx_encoder_set_timing", self.h, int(bool(on)))

    def stage_ms(self):
        ms = np.zeros(32, np.float32)
        n = lib().ulcx_encoder_stage_ms(self.h, _p(ms, _f32p), 32)
        return {lib().ulcx_encoder_stage_name(i).decode(): float(ms[i]) for i in range(n)}


class BatchDecoder(_StreamSlots):
    _kind = "decoder"

    def __init__(self, n_streams, n_chan, block_size, max_blocks, device=0):
        self.B, self.C, self.BS, self.maxK = n_streams, n_chan, block_size, max_blocks
        self.h = C.c_void_p()
        _call("ulcx_decoder_create", C.byref(self.h), device, n_streams, n_chan, block_size, max_blocks)

    def close(self):
        if self.h:
            lib().ulcx_decoder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_cut(self):
        """(workgroups of the last call's synthesis or 0 = one per stream, leading whole-stream workgroups, resident workgroups)"""
        g, f, r = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _call("ulcx_decoder_last_cut", self.h, C.byref(g), C.byref(f), C.byref(r))
        return g.value, f.value, r.value

    def reset(self):
        _call("ulcx_decoder_reset", self.h)

    def _pcm_out(self, n, n_blocks):
        """The block-order outputs, zeroed -> (pcm [n][n_blocks * BS][C], bits [n][n_blocks])."""
        return np.zeros((n, n_blocks * self.BS, self.C), np.float32), np.zeros((n, n_blocks), np.int32)

    def decode(self, blocks):
        """blocks: uint8 [B][K][slot] -> (pcm [B][K*BS][C], bits [B][K])."""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        B, K, slot = blocks.shape
        assert B == self.B
        pcm, bits = self._pcm_out(B, K)
        _call("ulcx_decode_host", self.h, _p(blocks, _u8p), slot, K, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def decode_packed(self, payload, payload_bytes, n_blocks):
        """payload: uint8 [B][stride] contiguous blocks per stream (a .ulc file's data section each);
        continues from where the previous call stopped."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        nbytes = np.ascontiguousarray(payload_bytes, dtype=np.int32)
        B, stride = payload.shape
        pcm, bits = self._pcm_out(B, n_blocks)
        _call("ulcx_decode_packed_host", self.h, _p(payload, _u8p), stride, _p(nbytes, _i32p), n_blocks, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def upload_payload(self, payload, payload_bytes):
        """Packed payloads to the device once (rewinds the read positions); decode_resident() then walks them."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        nbytes = np.ascontiguousarray(payload_bytes, dtype=np.int32)
        _call("ulcx_decoder_upload_payload", self.h, _p(payload, _u8p), payload.shape[1], _p(nbytes, _i32p))

    def decode_resident(self, n_blocks):
        pcm, bits = self._pcm_out(self.B, n_blocks)
        _call("ulcx_decode_resident_host", self.h, n_blocks, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def index_packed(self, payload, payload_bytes, max_blocks):
        """Block index of packed payloads: (index [B][max_blocks+1] of INDEX_DTYPE, n_blocks [B]).  Entry k of a stream is
        the byte at which its block k starts and the noise generator's state there; entry n_blocks[s] closes the table,
        later ones are (-1, 0).  No stream state is read or changed."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        nbytes = np.ascontiguousarray(payload_bytes, dtype=np.int32)
        B, stride = payload.shape
        assert B == self.B
        index = np.zeros((B, max_blocks + 1), INDEX_DTYPE)
        count = np.zeros(B, np.int32)
        _call("ulcx_index_packed_host", self.h, _p(payload, _u8p), stride, _p(nbytes, _i32p), max_blocks, index.ctypes.data, _p(count, _i32p))
        return index, count

    def decode_range(self, payload, payload_bytes, index, index_blocks, first, n_blocks):
        """Blocks first[s] .. first[s]+n_blocks-1 of every stream -> (pcm [B][n_blocks*BS][C], bits [B][n_blocks]), as a
        sequential decode from block 0 gives them; n_blocks <= max_blocks - 1.  The streams' state afterwards is that of a
        sequential decode up to the range's last block."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        nbytes = np.ascontiguousarray(payload_bytes, dtype=np.int32)
        index = np.ascontiguousarray(index, dtype=INDEX_DTYPE)
        count = np.ascontiguousarray(index_blocks, dtype=np.int32)
        first = np.ascontiguousarray(first, dtype=np.int32)
        B, stride = payload.shape
        assert B == self.B and index.shape[0] == B and count.shape == (B,) and first.shape == (B,)
        pcm, bits = self._pcm_out(B, n_blocks)
        _call("ulcx_decode_range_host", self.h, _p(payload, _u8p), stride, _p(nbytes, _i32p), index.ctypes.data, index.shape[1], _p(count, _i32p),
              _p(first, _i32p), n_blocks, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def index_resident(self, max_blocks):
        """Index the payloads uploaded with upload_payload() and keep the index in the decoder -> n_blocks [B]."""
        count = np.zeros(self.B, np.int32)
        _call("ulcx_decoder_index_resident", self.h, max_blocks, _p(count, _i32p))
        return count

    def decode_resident_range(self, first, n_blocks):
        first = np.ascontiguousarray(first, dtype=np.int32)
        assert first.shape == (self.B,)
        pcm, bits = self._pcm_out(self.B, n_blocks)
        _call("ulcx_decode_resident_range_host", self.h, _p(first, _i32p), n_blocks, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def index_begin_dev(self, n_rows, d_index, index_stride, d_n_blocks, stream=0):
        """Open an index of n_rows rows on the device (entry 0 = (0, 1234567), the rest (-1, 0), counts 0)."""
        _dev_call("ulcx_index_begin_dev", False, stream, self.h, n_rows, d_index, index_stride, d_n_blocks)

    def index_slots_dev(self, n_rows, d_slots, slot, d_bits, n_blocks, d_index, index_stride, d_n_blocks, stream=0):
        """Append the n_blocks blocks of a slot-form buffer (what an encode call wrote: d_slots [n_rows][n_blocks][slot],
        d_bits [n_rows][n_blocks]) to each row's index; n_rows is the call's own, not the decoder's stream count."""
        _dev_call("ulcx_index_slots_dev", False, stream, self.h, n_rows, d_slots, slot, d_bits, n_blocks, d_index, index_stride, d_n_blocks)

    def index_slots(self, blocks, bits, index=None, n_blocks=None, index_stride=None):
        """Host form: blocks uint8 [R][K][slot], bits [R][K] -> (index [R][index_stride], n_blocks [R]).  Without `index` a new
        one of index_stride entries per row (default K + 1) is opened; with it, the call appends behind n_blocks[r]."""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        bits = np.ascontiguousarray(bits, dtype=np.int32)
        R, K, slot = blocks.shape
        assert bits.shape == (R, K)
        if index is None:
            index = new_index(R, index_stride or K + 1)
            count = np.zeros(R, np.int32)
        else:
            index = np.ascontiguousarray(index, dtype=INDEX_DTYPE).copy()
            count = np.ascontiguousarray(n_blocks, dtype=np.int32).copy()
            assert index.shape[0] == R and count.shape == (R,)
        _call("ulcx_index_slots_host", self.h, R, _p(blocks, _u8p), slot, _p(bits, _i32p), K, index.ctypes.data, index.shape[1], _p(count, _i32p))
        return index, count

    def set_resident_index(self, index, n_blocks):
        """Install a stored index for the payloads uploaded with upload_payload() (checked against their sizes first)."""
        index = np.ascontiguousarray(index, dtype=INDEX_DTYPE)
        count = np.ascontiguousarray(n_blocks, dtype=np.int32)
        assert index.shape[0] == self.B and count.shape == (self.B,)
        _call("ulcx_decoder_set_resident_index", self.h, index.ctypes.data, index.shape[1], _p(count, _i32p))

    def index_packed_dev(self, d_payload, stride, d_payload_bytes, max_blocks, d_index, d_n_blocks, stream=0):
        _dev_call("ulcx_index_packed_dev", False, stream, self.h, d_payload, stride, d_payload_bytes, max_blocks, d_index, d_n_blocks)

    def decode_range_dev(self, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, d_first, n_blocks, d_pcm, d_bits,
                         stream=0, pcm16=False):
        _dev_call("ulcx_decode_range_dev", pcm16, stream, self.h, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, d_first,
                  n_blocks, d_pcm, d_bits)

    # ---- The families over a corpus.  Each has one host body, which takes the layout and the corpus as _corpus_view() does:
    # strided (payload, payload_bytes, index, None, index_blocks), ragged (payload, payload_offs, index, index_offs, index_blocks).

    def _corpus_call(self, family, ragged, corpus, *tail):
        """ulcx_<family>[_ragged]_host on a corpus: handle, F and the corpus's argument run, then `tail`."""
        F, src = _corpus_view(ragged, *corpus)
        _call(f"ulcx_{family}{'_ragged' if ragged else ''}_host", self.h, F, *src, *tail)

    def _crops(self, ragged, corpus, files, first, n_blocks, count):
        n, rows = _row_view(files, first, np.int32, count)
        pcm, bits = self._pcm_out(n, n_blocks)
        self._corpus_call("decode_crops", ragged, corpus, *rows, n_blocks, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def _crops_samples(self, ragged, corpus, files, start, n_samples, length, lowrate=None, part=None):
        n, rows = _row_view(files, start, np.int64, length)
        planes = self.C if part is None else max(1, part_channels(self.C, part))              # (a bad part: the call refuses it)
        pcm = np.zeros((n, planes, max(1, n_samples)), np.float32)
        bs = self.BS if lowrate is None else (lowrate_block(self.BS, lowrate) or self.BS)     # (a bad ratio: the call refuses it)
        bits = np.zeros((n, max(1, crop_blocks(bs, n_samples))), np.int32)
        if part is not None:
            self._corpus_call("decode_crops_part", ragged, corpus, *rows, n_samples, int(lowrate or 0), int(part), _p(pcm, _f32p), _p(bits, _i32p))
        elif lowrate is None:
            self._corpus_call("decode_crops_samples", ragged, corpus, *rows, n_samples, _p(pcm, _f32p), _p(bits, _i32p))
        else:
            self._corpus_call("decode_crops_lowrate", ragged, corpus, *rows, n_samples, int(lowrate), _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def _crops_spectra(self, ragged, corpus, files, first, n_blocks, count, flags):
        n, rows = _row_view(files, first, np.int32, count)
        coef = np.zeros((n, self.C, n_blocks, self.BS), np.float32)
        wc = np.zeros((n, n_blocks), np.int32)
        bits = np.zeros((n, n_blocks), np.int32)
        self._corpus_call("decode_crops_spectra", ragged, corpus, *rows, n_blocks, int(flags), _p(coef, _f32p), _p(wc, _i32p), _p(bits, _i32p))
        return coef, wc, bits

    def _crops_distortion(self, ragged, corpus, files, first, n_blocks, ref, ref_row, ref_first, count, n_seg, flags):
        n, rows = _row_view(files, first, np.int32, count)
        n_ref = n_ref_blocks = 0
        if ref is not None:
            ref = np.ascontiguousarray(ref, dtype=np.float32)
            assert ref.ndim == 4 and ref.shape[1] == self.C and ref.shape[3] == self.BS
            n_ref, n_ref_blocks = ref.shape[0], ref.shape[2]
        row = None if ref_row is None else np.ascontiguousarray(ref_row, dtype=np.int32)
        rfirst = None if ref_first is None else np.ascontiguousarray(ref_first, dtype=np.int32)
        assert (row is None or row.shape == (n,)) and (rfirst is None or rfirst.shape == (n,))
        dist = np.zeros((n, self.C, n_blocks, max(int(n_seg), 1), 3), np.float64)
        wc = np.zeros((n, n_blocks), np.int32)
        bits = np.zeros((n, n_blocks), np.int32)
        self._corpus_call("decode_crops_distortion", ragged, corpus, *rows, n_blocks, _p(ref, _f32p), n_ref, n_ref_blocks, _p(row, _i32p),
                          _p(rfirst, _i32p), int(n_seg), int(flags), _p(dist, _f64p), _p(wc, _i32p), _p(bits, _i32p))
        return dist, wc, bits

    def _splice(self, ragged, corpus, segments, out_payload_stride, out_index_stride, out):
        offs, seg = segments if isinstance(segments, tuple) else self._segments(segments)
        offs = np.ascontiguousarray(offs, dtype=np.int32)
        seg = np.ascontiguousarray(seg, dtype=SEGMENT_DTYPE)
        n_out, n_seg = offs.shape[0] - 1, seg.shape[0]
        r = out or {"payload": np.zeros((n_out, out_payload_stride), np.uint8), "payload_bytes": np.zeros(n_out, np.int32),
                    "max_block": np.zeros(n_out, np.int32), "index": np.zeros((n_out, out_index_stride), INDEX_DTYPE),
                    "index_blocks": np.zeros(n_out, np.int32), "seg_start": np.zeros(n_seg, np.int32)}
        self._corpus_call("corpus_splice", ragged, corpus, n_out, _p(offs, _i32p), seg.ctypes.data, n_seg, _p(r["payload"], _u8p),
                          r["payload"].shape[1], _p(r["payload_bytes"], _i32p), _p(r["max_block"], _i32p), r["index"].ctypes.data,
                          r["index"].shape[1], _p(r["index_blocks"], _i32p), _p(r["seg_start"], _i32p))
        return r

    def decode_crops(self, payload, payload_bytes, index, index_blocks, files, first, n_blocks, count=None):
        """Crops of a corpus: payload uint8 [F][stride], payload_bytes [F], index [F][index_stride], index_blocks [F]; row i of
        the result is blocks first[i] .. first[i]+n_blocks-1 of file files[i] (its leading count[i] blocks when `count` is
        given) -> (pcm [n][n_blocks*BS][C], bits [n][n_blocks]), as a sequential decode of that file from block 0 gives them.
        n <= n_streams, n_blocks <= max_blocks - 1; F is the corpus's own.  No stream's state is read or changed."""
        return self._crops(False, (payload, payload_bytes, index, None, index_blocks), files, first, n_blocks, count)

    def decode_crops_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_first, d_count,
                         n_blocks, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_count 0 / None: every row takes all n_blocks); d_pcm is int16 [n][n_blocks][BS][C] with pcm16."""
        _dev_call("ulcx_decode_crops_dev", pcm16, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks,
                  n, d_file, d_first, d_count or None, n_blocks, d_pcm, d_bits)

    @staticmethod
    def _segments(segments):
        """One list of (file, first, count) per output file -> (seg_offs int32 [nOut + 1], seg SEGMENT_DTYPE [nSeg])."""
        offs = np.zeros(len(segments) + 1, np.int32)
        offs[1:] = np.cumsum([len(f) for f in segments])
        seg = np.zeros(max(int(offs[-1]), 1), SEGMENT_DTYPE)
        flat = [tuple(int(x) for x in g) for f in segments for g in f]
        if flat:
            seg[:len(flat)] = np.array(flat, SEGMENT_DTYPE)
        return offs, seg

    def corpus_splice(self, payload, payload_bytes, index, index_blocks, segments, out_payload_stride, out_index_stride, out=None):
        """New files from block ranges of a corpus's files (ulcx_corpus_splice_host).  The source as decode_crops() takes it;
        `segments` is one list of (file, first, count) per output file, or the pair (seg_offs int32 [nOut + 1], seg SEGMENT_DTYPE
        [nSeg]).  -> dict: payload uint8 [nOut][out_payload_stride] (bytes behind payload_bytes[o] as `out` held them, or zeros),
        payload_bytes, max_block, index [nOut][out_index_stride], index_blocks, seg_start [nSeg]."""
        return self._splice(False, (payload, payload_bytes, index, None, index_blocks), segments, out_payload_stride, out_index_stride, out)

    def corpus_splice_ragged(self, payload, payload_offs, index, index_offs, index_blocks, segments, out_payload_stride, out_index_stride, out=None):
        """corpus_splice() of a ragged source (ulcx_corpus_splice_ragged_host), as decode_crops_ragged() takes it; the output is strided."""
        return self._splice(True, (payload, payload_offs, index, index_offs, index_blocks), segments, out_payload_stride, out_index_stride, out)

    def corpus_splice_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n_out, d_seg_offs, d_seg, n_seg,
                          d_out_payload, out_payload_stride, d_out_payload_bytes, d_out_max_block, d_out_index, out_index_stride, d_out_index_blocks,
                          d_seg_start, stream=0):
        """Device form (raw device pointers; d_out_max_block 0 / None: not wanted); asynchronous on `stream`."""
        _dev_call("ulcx_corpus_splice_dev", False, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks,
                  n_out, d_seg_offs, d_seg, n_seg, d_out_payload, out_payload_stride, d_out_payload_bytes, d_out_max_block or None, d_out_index,
                  out_index_stride, d_out_index_blocks, d_seg_start)

    def corpus_splice_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks, n_out,
                                 d_seg_offs, d_seg, n_seg, d_out_payload, out_payload_stride, d_out_payload_bytes, d_out_max_block, d_out_index,
                                 out_index_stride, d_out_index_blocks, d_seg_start, stream=0):
        _dev_call("ulcx_corpus_splice_ragged_dev", False, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n_out, d_seg_offs, d_seg, n_seg, d_out_payload, out_payload_stride, d_out_payload_bytes,
                  d_out_max_block or None, d_out_index, out_index_stride, d_out_index_blocks, d_seg_start)

    def index_packed_rows(self, payload, payload_bytes, max_blocks):
        """index_packed() for any number of rows (a corpus's files), whatever the decoder's stream count."""
        R, src = _payload_view(False, payload, payload_bytes)
        index = np.zeros((R, max_blocks + 1), INDEX_DTYPE)
        count = np.zeros(R, np.int32)
        _call("ulcx_index_packed_rows_host", self.h, R, *src, max_blocks, index.ctypes.data, _p(count, _i32p))
        return index, count

    def index_packed_rows_dev(self, n_rows, d_payload, stride, d_payload_bytes, max_blocks, d_index, d_n_blocks, stream=0):
        _dev_call("ulcx_index_packed_rows_dev", False, stream, self.h, n_rows, d_payload, stride, d_payload_bytes, max_blocks, d_index, d_n_blocks)

    def decode_crops_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, first, n_blocks, count=None):
        """decode_crops() of a ragged corpus: payload uint8 [total], the files back to back, file f its bytes payload_offs[f] ..
        payload_offs[f+1] (int64 [F+1]); index [entries], row f its entries index_offs[f] .. index_offs[f+1] (int64 [F+1]);
        index_blocks [F].  Rows, counts and the result as decode_crops()."""
        return self._crops(True, (payload, payload_offs, index, index_offs, index_blocks), files, first, n_blocks, count)

    def decode_crops_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                n, d_file, d_first, d_count, n_blocks, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_count 0 / None: every row takes all n_blocks); d_pcm is int16 [n][n_blocks][BS][C] with pcm16."""
        _dev_call("ulcx_decode_crops_ragged_dev", pcm16, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n, d_file, d_first, d_count or None, n_blocks, d_pcm, d_bits)

    def decode_crops_spectra(self, payload, payload_bytes, index, index_blocks, files, first, n_blocks, count=None, flags=0):
        """decode_crops() stopped in front of the inverse transform (ulcx_decode_crops_spectra_host): the dequantised MDCT
        coefficients of the same rows, noise included -> (coef [n][C][n_blocks][BS], wc [n][n_blocks], bits [n][n_blocks]).
        flags: 0, or SPECTRA_LR (channel pairs as m + s, m - s)."""
        return self._crops_spectra(False, (payload, payload_bytes, index, None, index_blocks), files, first, n_blocks, count, flags)

    def decode_crops_spectra_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_first, d_count,
                                 n_blocks, flags, d_coef, d_wc, d_bits, stream=0):
        """Device form (d_count 0 / None: every row takes all n_blocks); d_coef float32 [n][C][n_blocks][BS], d_wc / d_bits [n][n_blocks]."""
        _dev_call("ulcx_decode_crops_spectra_dev", False, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride,
                  d_index_blocks, n, d_file, d_first, d_count or None, n_blocks, int(flags), d_coef, d_wc, d_bits)

    def synth_spectra(self, coef, wc, flags=0):
        """PCM from caller-held MDCT planes through the decoder's inverse transform (ulcx_synth_spectra_host): coef float32
        [n][C][n_blocks][BS] and wc int32 [n][n_blocks] as the spectra and clip-spectra calls write them -> (pcm [n][C][n_out * BS],
        live [n][n_out]), n_out = n_blocks - 1 with SYNTH_WARM (plane 0 is the block in front: no output), else n_blocks.
        flags: SPECTRA_LR (the planes hold left/right: no un-mix), SYNTH_WARM."""
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        wc = np.ascontiguousarray(wc, dtype=np.int32)
        assert coef.ndim == 4 and coef.shape[1] == self.C and coef.shape[3] == self.BS and wc.shape == (coef.shape[0], coef.shape[2])
        n, n_blocks = wc.shape
        n_out = max(1, n_blocks - (1 if int(flags) & SYNTH_WARM else 0))
        pcm = np.zeros((n, self.C, n_out * self.BS), np.float32)
        live = np.zeros((n, n_out), np.int32)
        _call("ulcx_synth_spectra_host", self.h, n, n_blocks, int(flags), _p(coef, _f32p), _p(wc, _i32p), _p(pcm, _f32p), _p(live, _i32p))
        return pcm, live

    def synth_spectra_dev(self, n, n_blocks, flags, d_coef, d_wc, d_pcm, d_live, stream=0, pcm16=False):
        """Device form, asynchronous on `stream`: d_coef float32 [n][C][n_blocks][BS], d_wc int32 [n][n_blocks] -> d_pcm
        [n][C][n_out * BS] (int16 with pcm16), d_live int32 [n][n_out]."""
        _dev_call("ulcx_synth_spectra_dev", pcm16, stream, self.h, n, n_blocks, int(flags), d_coef, d_wc, d_pcm, d_live)

    def decode_crops_spectra_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, first, n_blocks, count=None, flags=0):
        """decode_crops_spectra() of a ragged corpus, held as for decode_crops_ragged()."""
        return self._crops_spectra(True, (payload, payload_offs, index, index_offs, index_blocks), files, first, n_blocks, count, flags)

    def decode_crops_spectra_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                        n, d_file, d_first, d_count, n_blocks, flags, d_coef, d_wc, d_bits, stream=0):
        """Device form of a ragged corpus (d_count 0 / None: every row takes all n_blocks)."""
        _dev_call("ulcx_decode_crops_spectra_ragged_dev", False, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n, d_file, d_first, d_count or None, n_blocks, int(flags), d_coef, d_wc, d_bits)

    def decode_crops_distortion(self, payload, payload_bytes, index, index_blocks, files, first, n_blocks, ref=None, ref_row=None, ref_first=None,
                                count=None, n_seg=1, flags=0):
        """decode_crops_spectra() summed against reference planes instead of returned (ulcx_decode_crops_distortion_host): per (row,
        channel, block, segment of BS / n_seg coefficients) the binary64 sums {S, Y, E} of the reference's, the coded spectrum's and the
        error's energy, added in one fixed order.  ref: float32 [n_ref][C][n_ref_blocks][BS] or None (S = 0, E = Y); ref_row[i] /
        ref_first[i]: the reference row of crop row i (None: i) and the reference block beside its output block 0 (None: 0).
        -> (dist float64 [n][C][n_blocks][n_seg][3], wc [n][n_blocks], bits [n][n_blocks])."""
        return self._crops_distortion(False, (payload, payload_bytes, index, None, index_blocks), files, first, n_blocks, ref, ref_row, ref_first,
                                      count, n_seg, flags)

    def decode_crops_distortion_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_first, d_count,
                                    n_blocks, d_ref, n_ref, n_ref_blocks, d_ref_row, d_ref_first, n_seg, flags, d_dist, d_wc, d_bits, stream=0):
        """Device form (d_count, d_ref, d_ref_row, d_ref_first 0 / None: not given); d_ref float32 [n_ref][C][n_ref_blocks][BS], d_dist
        float64 [n][C][n_blocks][n_seg][3], d_wc / d_bits [n][n_blocks]."""
        _dev_call("ulcx_decode_crops_distortion_dev", False, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride,
                  d_index_blocks, n, d_file, d_first, d_count or None, n_blocks, d_ref or None, n_ref, n_ref_blocks, d_ref_row or None,
                  d_ref_first or None, int(n_seg), int(flags), d_dist, d_wc, d_bits)

    def decode_crops_distortion_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, first, n_blocks, ref=None, ref_row=None,
                                       ref_first=None, count=None, n_seg=1, flags=0):
        """decode_crops_distortion() of a ragged corpus, held as for decode_crops_ragged()."""
        return self._crops_distortion(True, (payload, payload_offs, index, index_offs, index_blocks), files, first, n_blocks, ref, ref_row, ref_first,
                                      count, n_seg, flags)

    def decode_crops_distortion_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                           n, d_file, d_first, d_count, n_blocks, d_ref, n_ref, n_ref_blocks, d_ref_row, d_ref_first, n_seg, flags,
                                           d_dist, d_wc, d_bits, stream=0):
        """Device form of a ragged corpus (d_count, d_ref, d_ref_row, d_ref_first 0 / None: not given)."""
        _dev_call("ulcx_decode_crops_distortion_ragged_dev", False, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index,
                  index_total, d_index_offs, d_index_blocks, n, d_file, d_first, d_count or None, n_blocks, d_ref or None, n_ref, n_ref_blocks,
                  d_ref_row or None, d_ref_first or None, int(n_seg), int(flags), d_dist, d_wc, d_bits)

    def decode_crops_samples(self, payload, payload_bytes, index, index_blocks, files, start, n_samples, length=None):
        """Sample crops of a corpus held as for decode_crops(): row i is n_samples samples from sample start[i] (int64) of the
        decoded stream of file files[i], its leading length[i] when `length` is given (zeros behind), channels-first
        -> (pcm [n][C][n_samples], bits [n][crop_blocks(BS, n_samples)])."""
        return self._crops_samples(False, (payload, payload_bytes, index, None, index_blocks), files, start, n_samples, length)

    def decode_crops_samples_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_start, d_len,
                                 n_samples, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_len 0 / None: every row takes all n_samples); d_pcm is [n][C][n_samples], int16 with pcm16."""
        _dev_call("ulcx_decode_crops_samples_dev", pcm16, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride,
                  d_index_blocks, n, d_file, d_start, d_len or None, n_samples, d_pcm, d_bits)

    def decode_crops_samples_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, start, n_samples, length=None):
        """decode_crops_samples() of a ragged corpus, held as for decode_crops_ragged()."""
        return self._crops_samples(True, (payload, payload_offs, index, index_offs, index_blocks), files, start, n_samples, length)

    def decode_crops_samples_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                        n, d_file, d_start, d_len, n_samples, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_len 0 / None: every row takes all n_samples); d_pcm is [n][C][n_samples], int16 with pcm16."""
        _dev_call("ulcx_decode_crops_samples_ragged_dev", pcm16, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n, d_file, d_start, d_len or None, n_samples, d_pcm, d_bits)

    # low-rate sample crops (include/ulc_amd_lowrate.h): the sample-crop calls on the stream reduced by 1 << lowrate - block size
    # BS >> lowrate, start and n_samples in reduced samples, reduced sample m at full-rate time D m + (D - 1) / 2

    def decode_crops_lowrate(self, payload, payload_bytes, index, index_blocks, files, start, n_samples, lowrate, length=None):
        """decode_crops_samples() at 1 / (1 << lowrate) of the file's rate, lowrate 0 .. 3 (0: that call, bit for bit)
        -> (pcm [n][C][n_samples], bits [n][crop_blocks(BS >> lowrate, n_samples)], the full blocks' sizes)."""
        return self._crops_samples(False, (payload, payload_bytes, index, None, index_blocks), files, start, n_samples, length, lowrate)

    def decode_crops_lowrate_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_start, d_len,
                                 n_samples, lowrate, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_len 0 / None: every row takes all n_samples); d_pcm is [n][C][n_samples], int16 with pcm16."""
        _dev_call("ulcx_decode_crops_lowrate_dev", pcm16, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride,
                  d_index_blocks, n, d_file, d_start, d_len or None, n_samples, int(lowrate), d_pcm, d_bits)

    def decode_crops_lowrate_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, start, n_samples, lowrate, length=None):
        """decode_crops_lowrate() of a ragged corpus, held as for decode_crops_ragged()."""
        return self._crops_samples(True, (payload, payload_offs, index, index_offs, index_blocks), files, start, n_samples, length, lowrate)

    # mid and side crops (include/ulc_amd_part.h): the low-rate calls over one coded channel of every pair - plane j of the output is
    # coded channel 2 j + part as it stands in front of the un-mix, part_channels(C, part) planes per row
    def decode_crops_part(self, payload, payload_bytes, index, index_blocks, files, start, n_samples, part, lowrate=0, length=None):
        """decode_crops_lowrate() of the mid (part = PART_MID) or side (PART_SIDE) channels alone
        -> (pcm [n][part_channels(C, part)][n_samples], bits as decode_crops_lowrate())."""
        return self._crops_samples(False, (payload, payload_bytes, index, None, index_blocks), files, start, n_samples, length, lowrate, part)

    def decode_crops_part_dev(self, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride, d_index_blocks, n, d_file, d_start, d_len,
                              n_samples, lowrate, part, d_pcm, d_bits, stream=0, pcm16=False):
        """ulcx_decode_crops_part_dev / _dev_pcm16 on raw device pointers (d_len: 0 for none)."""
        _dev_call("ulcx_decode_crops_part_dev", pcm16, stream, self.h, n_files, d_payload, stride, d_payload_bytes, d_index, index_stride,
                  d_index_blocks, n, d_file, d_start, d_len or None, n_samples, int(lowrate), int(part), d_pcm, d_bits)

    def decode_crops_part_ragged(self, payload, payload_offs, index, index_offs, index_blocks, files, start, n_samples, part, lowrate=0, length=None):
        """decode_crops_part() of a ragged corpus, held as for decode_crops_ragged()."""
        return self._crops_samples(True, (payload, payload_offs, index, index_offs, index_blocks), files, start, n_samples, length, lowrate, part)

    def decode_crops_part_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                     n, d_file, d_start, d_len, n_samples, lowrate, part, d_pcm, d_bits, stream=0, pcm16=False):
        """ulcx_decode_crops_part_ragged_dev / _dev_pcm16 on raw device pointers (d_len: 0 for none)."""
        _dev_call("ulcx_decode_crops_part_ragged_dev", pcm16, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n, d_file, d_start, d_len or None, n_samples, int(lowrate), int(part), d_pcm, d_bits)

    def decode_crops_lowrate_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_index_blocks,
                                        n, d_file, d_start, d_len, n_samples, lowrate, d_pcm, d_bits, stream=0, pcm16=False):
        """Device form (d_len 0 / None: every row takes all n_samples); d_pcm is [n][C][n_samples], int16 with pcm16."""
        _dev_call("ulcx_decode_crops_lowrate_ragged_dev", pcm16, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_index_blocks, n, d_file, d_start, d_len or None, n_samples, int(lowrate), d_pcm, d_bits)

    def index_packed_ragged(self, payload, payload_offs, index_offs, index=None):
        """The index of files back to back: row f (entries index_offs[f] .. index_offs[f+1]) as index_packed_rows() fills a row of
        that capacity - 1 blocks.  -> (index [index_offs[-1]], or `index` filled in place: entries outside the rows stay; count [F])."""
        F, src = _payload_view(True, payload, payload_offs)
        ioffs = np.ascontiguousarray(index_offs, dtype=np.int64)
        assert F >= 1 and ioffs.shape == (F + 1,)
        if index is None:
            index = np.zeros(max(0, int(ioffs.max())), INDEX_DTYPE)
        assert index.dtype == INDEX_DTYPE and index.ndim == 1 and index.flags["C_CONTIGUOUS"]
        count = np.zeros(F, np.int32)
        _call("ulcx_index_packed_ragged_host", self.h, F, *src, index.ctypes.data, index.size, _p(ioffs, _i64p), _p(count, _i32p))
        return index, count

    def index_packed_ragged_dev(self, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total, d_index_offs, d_n_blocks, stream=0):
        _dev_call("ulcx_index_packed_ragged_dev", False, stream, self.h, n_files, d_payload, payload_total, d_payload_offs, d_index, index_total,
                  d_index_offs, d_n_blocks)

    def decode_packed_dev(self, d_payload, stride, d_payload_bytes, n_blocks, d_pcm, d_bits, stream=0):
        _dev_call("ulcx_decode_packed_dev", False, stream, self.h, d_payload, stride, d_payload_bytes, n_blocks, d_pcm, d_bits)

    def decode_dev(self, d_in, slot, n_blocks, d_pcm, d_bits, stream=0):
        _dev_call("ulcx_decode_dev", False, stream, self.h, d_in, slot, n_blocks, d_pcm, d_bits)

    def decode_dev_pcm16(self, d_in, slot, n_blocks, d_pcm16, d_bits, stream=0):
        """PCM16 output: d_pcm16 is a device pointer to int16 [B][K][BS][C]; converted on store as tools/WavIO_Helper.c:56-63."""
        _dev_call("ulcx_decode_dev", True, stream, self.h, d_in, slot, n_blocks, d_pcm16, d_bits)

    def decode_subset(self, slots, blocks):
        """As decode() for the listed slots only: blocks uint8 [n][K][slot], row i for slot slots[i]."""
        s, sp = self._slots(slots)
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        n, K, slot = blocks.shape
        assert n == s.size
        pcm, bits = self._pcm_out(n, K)
        _call("ulcx_decode_host_subset", self.h, sp, n, _p(blocks, _u8p), slot, K, _p(pcm, _f32p), _p(bits, _i32p))
        return pcm, bits

    def decode_subset_dev(self, d_slots, n, d_in, slot, n_blocks, d_pcm, d_bits, stream=0, pcm16=False):
        _dev_call("ulcx_decode_dev_subset", pcm16, stream, self.h, d_slots, n, d_in, slot, n_blocks, d_pcm, d_bits)

    def set_timing(self, on):
        _call("ulcx_decoder_set_timing", self.h, int(bool(on)))

    def stage_ms(self):
        ms = np.zeros(8, np.float32)
        n = lib().ulcx_decoder_stage_ms(self.h, _p(ms, _f32p), 8)
        return {lib().ulcx_decoder_stage_name(i).decode(): float(ms[i]) for i in range(n)}
