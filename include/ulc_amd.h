/*
 * ulc_amd.h — C ABI of libulc_amd.so, the MI355X (gfx950) implementation of the
 * ulc-codec per-block hot path.  Plain C, plain pointers and sizes; no torch, no
 * C++ types.  Two layers:
 *
 *  1. DROP-IN layer: the reference's own public API, same symbols, same struct
 *     layout (size/offsets are ABI: ULC_EncoderState_t = 104 bytes,
 *     ULC_DecoderState_t = 48 bytes on x86-64), same return conventions, so
 *     /root/reference/tools/ulcEncodeTool.c and ulcDecodeTool.c compile against the
 *     reference's own headers and link against this library unchanged.
 *     Replaces: /root/reference/include/ulcEncoder.h:47-78,85-88,135-137 and
 *               /root/reference/include/ulcDecoder.h:13-32,39-42,56
 *     (implemented by /root/reference/libulc/ulcEncoder.c:25-158 and ulcDecoder.c:26-302).
 *     Each call is a batch of one stream x one block through the batched path below.
 *
 *  2. BATCHED layer (ulcx_*): B independent streams x K consecutive blocks per
 *     call, state resident in HBM between calls.  This is what bench.py measures.
 *     It is what a maintainer would bind from ulcEncodeTool.c's block loop
 *     (tools/ulcEncodeTool.c:133-169) when encoding many files at once
 *     (INTEGRATION.md).
 *
 * Every entry point fails loudly (negative return + ulcx_last_error()) when no
 * gfx950 device / HIP runtime is usable — there is no CPU fallback in this library.
 */
#ifndef ULC_AMD_H
#define ULC_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* 1. Drop-in layer (reference ABI)                                           */
/* ------------------------------------------------------------------------- */
#ifndef ULC_AMD_NO_DROPIN_TYPES
struct ULC_TransientData_t { float Sum, SumW; };           /* ulcEncoder.h:44-46 */

/* ulcEncoder.h:47-78.  Caller sets RateHz/nChan/BlockSize, then Init.  The
 * pointer fields are private to the library: BufferData owns the (host) block,
 * TransformTemp receives each encoded block (the pointer the EncodeBlock calls
 * return), BlockComplexity is readable after each call (ulcEncodeTool.c:164). */
struct ULC_EncoderState_t {
    int    RateHz;
    int    nChan;
    int    BlockSize;
    int    WindowCtrl;
    int    NextWindowCtrl;
    float  BlockComplexity;
    float  TransientFilter[3];
    void  *BufferData;
    float *SampleBuffer;
    float *TransformBuffer;
    float *TransformNoise;
    float *TransformFwdLap;
    float *TransformTemp;
    int   *TransformIndex;
    struct ULC_TransientData_t *TransientBuffer;
};

/* ulcDecoder.h:13-32 */
struct ULC_DecoderState_t {
    int    nChan;
    int    BlockSize;
    int    LastSubBlockSize;
    void  *BufferData;
    float *TransformBuffer;
    float *TransformTemp;
    float *TransformInvLap;
};
#endif

/* ulcEncoder.h:85-88 / ulcEncoder.c:25-88.  Returns 1 on success, -1 on failure
 * (bad nChan/BlockSize, out of memory, or no usable GPU). */
int  ULC_EncoderState_Init(struct ULC_EncoderState_t *State);
void ULC_EncoderState_Destroy(struct ULC_EncoderState_t *State);

/* ulcEncoder.h:135-137 / ulcEncoder.c:93-158.  SrcData: BlockSize*nChan
 * interleaved floats.  Returns a pointer valid until the next call on State;
 * *Size (may be NULL) = bits, multiple of 8. */
const void *ULC_EncodeBlock_CBR(struct ULC_EncoderState_t *State, const float *SrcData, int *Size, float RateKbps);
const void *ULC_EncodeBlock_ABR(struct ULC_EncoderState_t *State, const float *SrcData, int *Size, float RateKbps, float AvgComplexity);
const void *ULC_EncodeBlock_VBR(struct ULC_EncoderState_t *State, const float *SrcData, int *Size, float Quality);

/* ulcDecoder.h:39-42,56 / ulcDecoder.c:26-302.  DecodeBlock returns bits
 * consumed (nybble granular), 0 = corrupt block. */
int  ULC_DecoderState_Init(struct ULC_DecoderState_t *State);
void ULC_DecoderState_Destroy(struct ULC_DecoderState_t *State);
int  ULC_DecodeBlock(struct ULC_DecoderState_t *State, float *DstData, const void *SrcBuffer);

/* Bytes of SrcBuffer that ULC_DecodeBlock (the reference's, ulcDecoder.c:82-216, and this library's) touches for the
 * block that starts there: a host-side walk of the block syntax that only counts.  Reads nothing at or past maxBytes and
 * returns at most maxBytes.  Host code, no GPU involved: ULC_DecodeBlock stages exactly this many bytes, and a
 * container reader can use it to index a .ulc payload (blocks carry no length, tools/ulcDecodeTool.c:153-165). */
int  ulcx_block_extent_bytes(const void *SrcBuffer, int nChan, int BlockSize, int maxBytes);
/* Round 3: the slot-form decoder cuts a call's (stream, block) pairs evenly over the synthesis workgroups when one workgroup
 * per stream would leave the device idle (few long streams).  This is the cut's arithmetic, exported for inspection and the
 * tests: the number of workgroups for nBlocks blocks of nStreams streams on a device that holds residentWG workgroups of the
 * synthesis kernel (1536 on an MI355X for stereo BlockSize 2048), or 0 = one workgroup per stream.  No reference counterpart
 * (the reference decodes one block per call, ulcDecoder.c:200-302). */
int  ulcx_dec_split_plan(int nStreams, int nBlocks, int residentWG);
/* Round 5: a batch of more streams than the device holds workgroups runs in rounds of one workgroup per stream; when the last
 * round is partly empty (4096 streams on 1536 resident workgroups) only ITS streams are cut, over the returned number of
 * workgroups at the end of the grid (0: no cut); *full receives the number of leading workgroups that take one whole stream
 * each.  Host arithmetic, exported for inspection and the tests.  No reference counterpart. */
int  ulcx_dec_tail_plan(int nStreams, int nBlocks, int residentWG, int *full);

/* ------------------------------------------------------------------------- */
/* 2. Batched layer                                                           */
/* ------------------------------------------------------------------------- */
typedef struct ulcx_encoder ulcx_encoder;
typedef struct ulcx_decoder ulcx_decoder;

enum {
    ULCX_OK            =  0,
    ULCX_ERR_ARG       = -1,   /* same validation as ulcEncoder.c:32-34 + batch limits */
    ULCX_ERR_NO_DEVICE = -2,   /* HIP runtime / gfx950 device not usable */
    ULCX_ERR_HIP       = -3,   /* a HIP call failed (message in ulcx_last_error) */
    ULCX_ERR_NOMEM     = -4,
    ULCX_ERR_UNSUPPORTED = -5  /* valid for the reference, not built for the device (no geometry is refused on this ground any more:
                                  BlockSize up to 32768 and up to 255 channels are accepted, as ulcEncoder.c:32-34 / ulcDecoder.c:33-35 do) */
};

enum { ULCX_MODE_VBR = 0, ULCX_MODE_CBR = 1, ULCX_MODE_ABR = 2 };

/* Caller buffers of the device-pointer entries (ulcx_*_dev*, ulcx_pack_streams_dev).  tests/test_gpu_buffer_contract.py holds
 * the library to every line of this: each call there runs on poisoned buffers between guards (tests/guarded_buffers.py).
 *
 * ALIGNMENT.  The widest access a kernel makes to the buffer; every row of a buffer keeps it (rows are multiples of it).
 *   16 bytes  binary32 samples: d_pcm of the encode, analyse, decode, decode_packed, decode_range and decode_crops calls
 *             (16-byte loads of the transform's fold, 16-byte stores of the stereo synthesis)
 *             binary32 coefficients: d_coef of the spectra calls (ulcx_decode_crops_spectra_*, ulcx_analyse_clips_*,
 *             ulcx_encode_clips_spectra_*: 16-byte stores)
 *             saved stream records: d_state of the stream-slot entries (16-byte loads and stores)
 *    8 bytes  PCM16 samples: d_pcm16 of the same calls (four samples per load / store);
 *             rate tables: d_rate, and ulcx_rung::rate of the _dev ladder forms (one 8-byte entry per load)
 *             offset tables: d_payloadOffs and d_indexOffs of the ragged-corpus calls (one int64 entry per load), and d_need
 *             of ulcx_corpus_ragged_dev
 *             sample positions: d_start of the sample-crop calls (one int64 entry per load)
 *    4 bytes  d_pcm of the sample-crop calls (ulcx_decode_crops_samples_*: a channel's plane starts at any sample; the kernels
 *             store two samples at once only where the address is a multiple of 8), and their d_len;
 *             d_pcm and d_len of the clip calls (ulcx_encode_clips_*: likewise, two samples per load only at a multiple of 8)
 *    2 bytes  d_pcm16 of the sample-crop calls (likewise; two samples at once only at a multiple of 4) and of the clip calls
 *    4 bytes  d_bits, d_wc, d_cplx, d_payloadBytes, d_maxBlock, d_nBlocks, d_indexBlocks, d_first, d_file, d_count, d_index (an entry is two
 *             4-byte words), and the slot lists of the stream-slot entries (their d_slots: int32 [n]);
 *             d_segOffs, d_seg (a segment is three 4-byte words) and d_segStart of the splice calls, and their d_out* tables
 *    none     the byte streams: d_out, d_in, d_payload and the d_slots of ulcx_pack_streams_dev and ulcx_index_slots_dev
 *             (slotBytes and payloadStride may be any positive value)
 *   A pointer that violates this makes the call return ULCX_ERR_ARG before any device work; the object's state is untouched
 *   and the next valid call continues as if the refused one had not been made.  (hipMalloc and the allocators built on it
 *   return 256-byte aligned memory: only pointers INTO an allocation can fail this.)
 *
 * EXTENT.  A call reads its inputs and writes its outputs, nothing else of the caller's: no byte in front of a buffer, none
 * behind the sizes given below for nBlocks (not maxBlocksPerCall) blocks, and no byte of an input.  Of the outputs
 *   d_bits, d_wc, d_cplx, d_pcm / d_pcm16, d_nBlocks, d_payloadBytes, d_maxBlock and the index are written in full: every
 *             element for nBlocks blocks - for a stream that ended (a corrupt block, the end of its payload) 0 bits and zero
 *             samples for every block from there on, whatever the buffer held; all maxBlocks + 1 index entries of a stream,
 *             the {-1, 0} ones behind the closing entry included
 *   d_out     bytes [0, d_bits / 8) of each slot are the block; the rest of the slot is NOT defined (today it keeps what the
 *             buffer held; no caller may rely on that): read a slot through its d_bits
 *   d_payload bytes [0, d_payloadBytes[s]) of stream s; the rest of payloadStride is not defined (not written).  The clip calls:
 *             the same per row, and all indexStride entries of every row of d_index.  ulcx_corpus_ragged_dev: bytes
 *             [0, d_payloadOffs[nFiles]) of d_outPayload and entries [0, d_indexOffs[nFiles]) of d_outIndex; both offset tables,
 *             d_outIndexBlocks and d_need in full; nothing behind payloadCap bytes / indexCap entries
 *   A NULL d_wc / d_cplx / d_maxBlock changes nothing else the call writes.
 *
 * ORDER.  Every call is enqueued on hipStream and returns without waiting for the device.  The private side streams it uses
 * have been joined back into hipStream by then, for reads of the inputs as for writes of the outputs: work enqueued on
 * hipStream after the call returns - a copy of the outputs, an overwrite of d_pcm with the next blocks - is ordered behind
 * all of it, with no event or synchronisation of the caller's.  Another stream needs an event recorded on hipStream.
 * A clip call's corpus (d_payload, d_payloadBytes, d_index, d_indexBlocks) may be handed to a crop call enqueued on hipStream
 * the moment the clip call returns; so may the tables of ulcx_corpus_ragged_dev. */

const char *ulcx_last_error(void);
int  ulcx_device_count(void);                 /* <= 0 when no usable device */
const char *ulcx_build_rev(void);             /* 12 hex digits: sha1 of the sources the library was built from (Makefile) */

/* Encoder for nStreams independent streams (all same RateHz/nChan/BlockSize);
 * at most maxBlocksPerCall blocks per stream per call.  device = HIP ordinal. */
int  ulcx_encoder_create(ulcx_encoder **enc, int device, int nStreams, int nChan, int BlockSize, int RateHz, int maxBlocksPerCall);
void ulcx_encoder_destroy(ulcx_encoder *enc);
int  ulcx_encoder_reset(ulcx_encoder *enc);   /* back to the state right after create */
int  ulcx_encoder_slot_bytes(const ulcx_encoder *enc);   /* bytes reserved per encoded block */

/* Encode nBlocks consecutive blocks of every stream.  All pointers are DEVICE
 * pointers; work is enqueued on hipStream (a hipStream_t, NULL = default stream)
 * and is asynchronous with respect to the host in every mode: nothing inside the call
 * waits for the device (the CBR/ABR rate search enqueues its full number of probe passes;
 * passes that find every block converged return at once on the device).  Internally the
 * call also uses private side streams, all joined back into hipStream before it returns.
 *   d_pcm  [nStreams][nBlocks][BlockSize][nChan] f32 interleaved (the layout the
 *          reference's EncodeBlock reads: ulcEncoder_BlockTransform.c:96-98)
 *   d_out  [nStreams][nBlocks][slot_bytes] encoded blocks, byte aligned, each
 *          identical to what ULC_EncodeBlock_* returns for that call
 *   d_bits [nStreams][nBlocks] int32 block size in bits (multiple of 8)
 *   d_wc   optional [nStreams][nBlocks] int32 State->WindowCtrl of that call
 *   d_cplx optional [nStreams][nBlocks] f32 State->BlockComplexity of that call
 * mode/param0/param1: VBR(Quality) | CBR(RateKbps) | ABR(RateKbps, AvgComplexity). */
int  ulcx_encode_dev(ulcx_encoder *enc, int mode, float param0, float param1,
                     const float *d_pcm, int nBlocks,
                     uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);

/* PCM16 ingest: as ulcx_encode_dev, with d_pcm16 [nStreams][nBlocks][BlockSize][nChan]
 * int16 interleaved.  Samples are converted on load exactly as the reference's WAV reader feeds
 * ULC_EncodeBlock_* (tools/WavIO_Helper.c:49-55: (float)x * 2^-15), so the stream is identical to
 * converting on the host and calling ulcx_encode_dev; the input traffic is halved. */
int  ulcx_encode_dev_pcm16(ulcx_encoder *enc, int mode, float param0, float param1,
                           const int16_t *d_pcm16, int nBlocks,
                           uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);

/* Host-pointer convenience (H2D, encode, D2H, synchronous). */
int  ulcx_encode_host(ulcx_encoder *enc, int mode, float param0, float param1,
                      const float *h_pcm, int nBlocks,
                      uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx);

/* Per-stream rate settings, in the reference tool's own argument convention (tools/ulcEncodeTool.c:157-159):
 *   RateKbps < 0           -> VBR, Quality = -RateKbps        (ULC_EncodeBlock_VBR)
 *   else AvgComplexity > 0 -> ABR(RateKbps, AvgComplexity)    (ULC_EncodeBlock_ABR)
 *   else                   -> CBR(RateKbps)                   (ULC_EncodeBlock_CBR)
 * Valid entries (what ulcEncodeTool.c:43-50 accepts): both values finite, RateKbps != 0, AvgComplexity >= 0. */
typedef struct ulcx_rate { float RateKbps; float AvgComplexity; } ulcx_rate;     /* 8 bytes */

/* As ulcx_encode_dev / ulcx_encode_dev_pcm16, with stream s encoded under d_rate[s] instead of one setting for the whole
 * batch.  d_rate is a DEVICE array [nStreams], read by the call's kernels (it is not a kernel argument): the call stays
 * asynchronous, and a caller may rewrite the table between calls (hipMemcpyAsync on the same stream).  A stream's setting
 * may change from one call to the next: window control, the lapping state and BlockComplexity do not depend on it, and
 * block k of stream s is encoded exactly as ULC_EncodeBlock_{VBR,CBR,ABR} encodes it with that call's entry for s.
 * The device cannot validate the table without a synchronisation: an invalid entry is the caller's error (that stream's
 * output is unspecified; nothing outside the call's buffers is read or written).
 * These calls always enqueue the rate search's full number of probe passes; a pass in which every block has converged
 * (VBR entries never search) returns at once on the device. */
int  ulcx_encode_dev_rates(ulcx_encoder *enc, const ulcx_rate *d_rate, const float *d_pcm, int nBlocks,
                           uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_encode_dev_pcm16_rates(ulcx_encoder *enc, const ulcx_rate *d_rate, const int16_t *d_pcm16, int nBlocks,
                                 uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
/* Host-pointer convenience (synchronous).  h_rate [nStreams] is validated first, as ulcEncodeTool.c:43-50 validates its
 * argument: a non-finite value, RateKbps == 0 or AvgComplexity < 0 returns ULCX_ERR_ARG before any device work, and the
 * encoder's state is untouched. */
int  ulcx_encode_host_rates(ulcx_encoder *enc, const ulcx_rate *h_rate, const float *h_pcm, int nBlocks,
                            uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx);

/* Ladder: nBlocks blocks of every stream under nRungs rate settings in ONE call - several encodings of the same audio for
 * adaptive delivery.  Window control, transform, complexity, Bark levels, noise spectrum and the state update run once;
 * selection and writer run once per rung.  The streams' state advances once, and rung r's blocks are byte for byte those of
 * an encoder of its own fed the same PCM since creation and called with rung r's setting.
 *   d_out  [nRungs][nStreams][nBlocks][slot_bytes]      d_bits [nRungs][nStreams][nBlocks]
 *   d_wc / d_cplx  optional, [nStreams][nBlocks], written once (they do not depend on a rate mode)
 * nRungs is 1 .. ULCX_MAX_RUNGS; a bad count, a bad mode in a scalar rung or a non-zero `reserved` returns ULCX_ERR_ARG before
 * any device work and leaves the encoder's state untouched.  A scalar rung behaves as ulcx_encode_dev does (VBR: one pass, no
 * probe launches), a table rung as ulcx_encode_dev_rates does (always the full number of probe passes).  Asynchronous on
 * hipStream like its siblings.  With nRungs == 1 the call writes what the plain call writes.  Ladder, plain, _rates and
 * analysis calls may be mixed freely on one encoder.  ulcx_pack_streams_dev takes rung r at d_out + r * nStreams * nBlocks * slot.
 * Test hooks after a ladder call: ulcx_encoder_debug_fetch's kept set and nout are the last rung's (coefficients, noise and
 * keys are the same for every rung); ulcx_encoder_last_fallbacks is the sum over the rungs, ulcx_encoder_debug_writer_flags the last rung's; the stage times cover rung 0's
 * first pass, everything behind it falls into "cbr_probe_passes". */
#define ULCX_MAX_RUNGS 8
/* One rung of a ladder call.  A HOST struct (the array is read during the call, not kept).
 * rate == NULL: one setting for the whole batch, as ulcx_encode_dev takes it (mode / param0 / param1).
 * rate != NULL: a per-stream table [nStreams] as ulcx_encode_dev_rates takes it (a DEVICE pointer in the _dev forms,
 *               a host pointer in the _host form); mode / param0 / param1 are then unused. */
typedef struct ulcx_rung { int32_t mode; float param0, param1; int32_t reserved; const ulcx_rate *rate; } ulcx_rung;  /* 24 bytes, rate at 16 */

int  ulcx_encode_dev_ladder      (ulcx_encoder *enc, const ulcx_rung *rungs, int nRungs, const float   *d_pcm,   int nBlocks,
                                  uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_encode_dev_pcm16_ladder(ulcx_encoder *enc, const ulcx_rung *rungs, int nRungs, const int16_t *d_pcm16, int nBlocks,
                                  uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
/* Host-pointer convenience (synchronous).  Every table is validated as ulcx_encode_host_rates validates its own, a scalar
 * rung's parameters by the same rule (finite, param0 != 0, param1 >= 0), before any device work. */
int  ulcx_encode_host_ladder     (ulcx_encoder *enc, const ulcx_rung *rungs, int nRungs, const float   *h_pcm,   int nBlocks,
                                  uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx);
int  ulcx_encoder_last_rungs(ulcx_encoder *enc);   /* rungs of the last encode call (1 for every other encode call, 0 after an analysis call) */

/* Analysis only: window control, MDCT and block complexity of nBlocks consecutive blocks of every stream.
 * No selection, no writer, no output slots.  d_wc / d_cplx as in ulcx_encode_dev ([nStreams][nBlocks]); at least one
 * of them non-NULL.  The streams' persistent state advances exactly as an encode call of the same blocks advances it:
 * analysis and encode calls may be mixed freely on one encoder, and ulcx_encoder_reset() after an analysis pass gives
 * the second pass of the reference tool's ABR workflow a fresh encoder (ulcEncodeTool.c:157-188).  The values are those
 * ulcx_encode_dev writes for the same input - State->WindowCtrl and State->BlockComplexity after the block - and do
 * not depend on a rate mode.  Asynchronous on hipStream like ulcx_encode_dev; nBlocks in 1 .. maxBlocksPerCall.
 * After an analysis call there are no intermediates of a "last call": ulcx_encoder_debug_fetch returns ULCX_ERR_ARG and
 * ulcx_encoder_last_fallbacks 0 until the next encode call; ulcx_encoder_stage_ms reports 0 for the stages that did not run. */
int  ulcx_analyse_dev      (ulcx_encoder *enc, const float   *d_pcm,   int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_analyse_dev_pcm16(ulcx_encoder *enc, const int16_t *d_pcm16, int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_analyse_host     (ulcx_encoder *enc, const float   *h_pcm,   int nBlocks, int32_t *h_wc, float *h_cplx);   /* synchronous */

/* Debug/parity taps (device->host copies of the intermediates of the LAST call;
 * what the reference keeps in State->TransformBuffer / TransformNoise / the final
 * importance keys).  Each array is [nStreams][nBlocks][nChan*BlockSize] f32; pass
 * NULL to skip.  keep: [nStreams][nBlocks][nChan*BlockSize] uint8 (1 = coefficient
 * rank < nOutCoef of the final pass). nout: [nStreams][nBlocks] int32. */
int  ulcx_encoder_debug_fetch(ulcx_encoder *enc, int nBlocks, float *h_coef, float *h_noise, float *h_keys,
                              uint8_t *h_keep, int32_t *h_nout);

/* Number of blocks of the last call (final pass) whose threshold tie group straddled the
 * cut and went through the exact heapsort emulation (BlockTransform.c:20-77).  Test hook. */
int  ulcx_encoder_last_fallbacks(ulcx_encoder *enc);
/* Test hooks, read-only: which capacity tier of the wave writer every block of the last encode call ended in, as the call's
 * final pass (of its last rung) left it.  h_flags [nStreams][nBlocks] (a subset call: its first n rows), per block
 *   bit 0: a unit overflowed the small capacities, the block left the first launch of k_encode_wave;
 *   bit 1: the block was left to the serial kernel k_encode_units (a retry launch could not hold it, or there is none);
 *   bit 2: the wave writer packed the block into its slot itself (stereo, un-decimated; k_pack passes).
 * Synchronises the device and copies; no kernel, no work in a call that does not ask.  Refuses (ULCX_ERR_ARG) before the first
 * encode call, after an analysis call and with an nBlocks other than the last call's.
 * _plan: the capacities {kept coefficients, zones, nybbles} of the small, the medium and the full tier this object launches
 * with, then haveMid (rate-search probes and the exact path retry on the medium tier, not on the full one) and haveFull (0: one
 * launch, no retry - what the small capacities cannot hold goes straight to the serial kernel). */
int  ulcx_encoder_debug_writer_flags(ulcx_encoder *enc, int nBlocks, int32_t *h_flags);
int  ulcx_encoder_debug_writer_plan(ulcx_encoder *enc, int32_t plan[11]);
/* Test hooks, read-only: the sample-rate axis.  RateHz decides at create time which Bark kernels an encoder runs: the band edges
 * of every subblock size follow from (BlockSize, RateHz), and the most bands the full-size tables have open at one line sizes
 * the snapshot ring of k_bark_uniform - 4 or 8, or 0 where more than 8 are open: then the lane-per-subblock kernels
 * (k_nbark / k_pbark) take every block.
 * ulcx_debug_band_plan: host arithmetic only, no device and no object; the code ulcx_encoder_create runs.  edges
 *   [2: noise | masking][4: subblock size BlockSize >> d][2: first line | end line][25 bands] int16; *most: the most bands open at
 *   one line (first line <= line <= end line) over both full-size tables; *ring: 0, 4 or 8.  most and ring may be NULL.
 * ulcx_debug_band_events: the same edges as the lists k_bark_uniform walks, [2][4][52] words line | kind << 16 | band << 24
 *   (kind 0: lower edge, 1: upper edge, 2: end of the subblock, 3: padding behind it).
 * ulcx_encoder_debug_plan: what this object decided - {ring, most bands open, k_nsums in use (useGapSums), the exact path's heap in
 *   LDS (0: in the object's scratch), resident workgroups of k_nsums, chunks of the window-control pipeline, selection with a wave
 *   per channel (k_select_pair)}.  No device work. */
int  ulcx_debug_band_plan(int BlockSize, int RateHz, int16_t *edges, int32_t *most, int32_t *ring);
int  ulcx_debug_band_events(int BlockSize, int RateHz, uint32_t *events);
int  ulcx_encoder_debug_plan(ulcx_encoder *enc, int32_t plan[7]);
/* Test hook, read-only: the window axis.  How a call of nBlocks on this object would be cut by the launch of its front half:
 * out = {transform chunks nCh, window-control steps nW, the nCh + 1 transform cuts, the nW + 1 step boundaries}, the rest of
 * the ULCX_FRONT_PLAN_WORDS words -1.  The plain launch (short calls, objects without side streams) reports one chunk and one
 * step, both {0, nBlocks}.  Host arithmetic by the function the launch calls; no device work.  Refuses (ULCX_ERR_ARG) an
 * nBlocks outside 1 .. maxBlocksPerCall. */
#define ULCX_FRONT_PLAN_WORDS 44
int  ulcx_encoder_debug_front_plan(ulcx_encoder *enc, int nBlocks, int32_t *out);
/* Test hook: how the last decode call's synthesis was launched - workgroups (0: one per stream), how many of them took one
 * whole stream each (ulcx_dec_tail_plan; 0 for an even cut, ulcx_dec_split_plan), and the workgroups of the synthesis kernel
 * the device holds at once (0: this geometry runs the general kernel, never cut). */
int  ulcx_decoder_last_cut(ulcx_decoder *dec, int *workgroups, int *wholeStreams, int *residentWG);
/* The cut of the last round for a range call (ulcx_decode_range_*): as ulcx_dec_tail_plan for calls of 24 blocks or more;
 * shorter calls (6 blocks or more, more streams than residentWG) are cut into pieces of max(2, nBlocks / 4) blocks - in a range
 * call a whole-stream workgroup runs the block in front of its range too, so a piece costs little more than it saves.
 * A range call of more streams than the device holds takes this plan before the even cut. */
int  ulcx_dec_range_tail_plan(int nStreams, int nBlocks, int residentWG, int *wholeStreams);
/* Test hook: from the next call on every `every`-th block of a call (block index % every == 0) is handed to the exact
 * heapsort path whether or not its threshold tie group straddles the cut (0 = off, the default).  The results must not
 * change: the full ranking decides the same kept set.  Exercises that path at a scale natural ties never reach. */
int  ulcx_encoder_debug_force_exact(ulcx_encoder *enc, int every);

int  ulcx_decoder_create(ulcx_decoder **dec, int device, int nStreams, int nChan, int BlockSize, int maxBlocksPerCall);
void ulcx_decoder_destroy(ulcx_decoder *dec);
int  ulcx_decoder_reset(ulcx_decoder *dec);

/* Decode nBlocks consecutive blocks of every stream (device pointers).
 *   d_in   [nStreams][nBlocks][slotBytes] encoded blocks (each starts at its slot; slotBytes need not exceed the
 *          largest block: nothing outside [d_in, d_in + nStreams*nBlocks*slotBytes) is read)
 *   d_pcm  [nStreams][nBlocks][BlockSize][nChan] f32 interleaved
 *          (ulcDecoder.c:291-297)
 *   d_bits [nStreams][nBlocks] int32 bits consumed per block; 0 = corrupt: that
 *          stream stops there (later blocks also report 0), like the tool aborting
 *          (tools/ulcDecodeTool.c:154-157). */
int  ulcx_decode_dev(ulcx_decoder *dec, const uint8_t *d_in, int slotBytes, int nBlocks,
                     float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_host(ulcx_decoder *dec, const uint8_t *h_in, int slotBytes, int nBlocks,
                      float *h_pcm, int32_t *h_bits);
/* One block of ONE stream per call, host pointers: what the drop-in ABI of section 1 does per ULC_EncodeBlock_* /
 * ULC_DecodeBlock call (encoder / decoder created with nStreams = 1, maxBlocksPerCall = 1).  The call's whole launch
 * sequence is captured into a HIP graph the first time (again when mode / parameters change) and replayed from pinned
 * staging buffers with one synchronisation; when capture is not possible the same sequence is enqueued directly.
 *   h_out     slot bytes (ulcx_encoder_slot_bytes)          stateOut  {WindowCtrl, NextWindowCtrl} and TransientFilter[3]
 *                                                                     as the reference leaves them in its state struct
 *                                                                     (ulcEncoder.h:57-64; BlockTransform.c:116-125)
 *   lastSubBlockSize  ulcDecoder.h:24 / ulcDecoder.c:300 */
int  ulcx_encode_block1(ulcx_encoder *enc, int mode, float param0, float param1, const float *h_pcm,
                        uint8_t *h_out, int32_t *bits, float *cplx, int32_t stateOut[2], float transientFilter[3]);
int  ulcx_decode_block1(ulcx_decoder *dec, const uint8_t *h_in, int nBytes, float *h_pcm, int32_t *bits, int32_t *lastSubBlockSize);
/* As ulcx_decode_block1 with the noise generator's state handed in and out.  The reference keeps that state in a
 * function-static word (libulc/ulcDecoder.c:75-81): one xorshift32 chain per PROCESS, shared by every decoder object, never
 * re-seeded by ULC_DecoderState_Init.  The drop-in of section 1 owns such a word and passes it here, so a process that
 * decodes several files one after the other draws the same noise as with the reference.  rngState NULL = the state stays
 * with the decoder object (what the batched entries do per stream). */
int  ulcx_decode_block1_rng(ulcx_decoder *dec, const uint8_t *h_in, int nBytes, float *h_pcm, int32_t *bits, int32_t *lastSubBlockSize,
                            uint32_t *rngState);

/* PCM16 output: as ulcx_decode_dev, writing d_pcm16 [nStreams][nBlocks][BlockSize][nChan]
 * int16, converted on store exactly as the reference's WAV writer does with ULC_DecodeBlock's output
 * (tools/WavIO_Helper.c:9-13,56-63: lrintf(clamp(x * 2^15, -32768, 32767))). */
int  ulcx_decode_dev_pcm16(ulcx_decoder *dec, const uint8_t *d_in, int slotBytes, int nBlocks,
                           int16_t *d_pcm16, int32_t *d_bits, void *hipStream);

/* Stream slots: per-stream reset, save / load and calls on a subset of an object's streams.
 * An object of nStreams streams has nStreams slots.  The entries above advance every slot in every call and the whole-object
 * reset rewinds all of them; the entries below work on the slots a list names, so that a slot whose stream has ended can
 * start another while its neighbours keep going, streams of different length share a batch without padding, and a stream
 * can be carried from one object (or device) to another mid-way.
 *   d_slots  DEVICE int32 [n], 4-byte aligned: slots of the object, n in 1 .. nStreams (h_slots of the host forms: a host array)
 *   d_state  DEVICE bytes [n][ulcx_*_stream_state_bytes], 16-byte aligned: one saved record per listed slot
 * All _dev forms are asynchronous on hipStream like their siblings and keep the ALIGNMENT / EXTENT / ORDER contract above
 * (a misaligned d_slots or d_state returns ULCX_ERR_ARG before any device work; save writes all n records in full).
 *
 * RESET.  A reset slot is in the state right after create: the next block fed to it is block 0 of a new stream.
 * SUBSET CALLS.  Row i of every buffer of the call belongs to slot d_slots[i] ([n][nBlocks]... instead of [nStreams][nBlocks]...);
 * only the listed slots' state is read and advanced.  Block k of the stream in slot s is byte for byte what
 * ULC_EncodeBlock_* / ULC_DecodeBlock writes for that stream fed on its own, every other slot's state is untouched, and
 * subset, plain, _rates, ladder, analysis, packed and range calls may be mixed freely on one object.  With d_slots = 0 ..
 * nStreams-1 a subset call writes what the plain call writes.  d_rate NULL: the scalar mode / param0 / param1; d_rate != NULL:
 * a device table [n] as ulcx_encode_dev_rates takes it, row i for slot d_slots[i].  A subset call gathers the listed slots'
 * state into a compact copy (allocated on the first such call, nStreams slots large), runs the plain call's kernels on it
 * and scatters the result back, all on hipStream.  Ladder, packed and range subset forms do not exist (yet).
 * SAVED RECORDS.  A record is a 16-byte header - uint32 magic, nChan, BlockSize, RateHz (0 in a decoder's record) - followed
 * by the stream's state: the encoder's two blocks of input history and window-control state; the decoder's lapping buffer,
 * LastSubBlockSize, noise generator, dead flag and packed read position.  ulcx_*_stream_state_bytes is a multiple of 16.
 * A record loads into any slot of any object of the same kind, nChan, BlockSize, RateHz and ulcx_build_rev(); nStreams,
 * maxBlocksPerCall and the device may differ (the bytes are plain: copy them through the host or peer to peer).  The host
 * load form refuses a record whose header does not match with ULCX_ERR_ARG; the device form leaves that slot as it was.
 * BAD LISTS.  The host forms refuse an entry outside [0, nStreams) and a duplicate entry with ULCX_ERR_ARG before any device
 * work, leaving the object untouched.  The device forms cannot refuse without a synchronisation: the row of an out-of-range
 * entry is processed from a fresh state and that state is discarded, save writes a fresh-state record for it, reset and load
 * skip it; with duplicate entries every row starts from the slot's state in front of the call and which row's state
 * remains is unspecified.  In every case nothing outside the call's buffers and the object is read or written. */
size_t ulcx_encoder_stream_state_bytes(const ulcx_encoder *enc);      /* 0 for NULL */
size_t ulcx_decoder_stream_state_bytes(const ulcx_decoder *dec);
int  ulcx_encoder_reset_streams_dev(ulcx_encoder *enc, const int32_t *d_slots, int n, void *hipStream);
int  ulcx_encoder_save_streams_dev (ulcx_encoder *enc, const int32_t *d_slots, int n, uint8_t *d_state, void *hipStream);
int  ulcx_encoder_load_streams_dev (ulcx_encoder *enc, const int32_t *d_slots, int n, const uint8_t *d_state, void *hipStream);
int  ulcx_decoder_reset_streams_dev(ulcx_decoder *dec, const int32_t *d_slots, int n, void *hipStream);
int  ulcx_decoder_save_streams_dev (ulcx_decoder *dec, const int32_t *d_slots, int n, uint8_t *d_state, void *hipStream);
int  ulcx_decoder_load_streams_dev (ulcx_decoder *dec, const int32_t *d_slots, int n, const uint8_t *d_state, void *hipStream);
int  ulcx_encode_dev_subset      (ulcx_encoder *enc, const int32_t *d_slots, int n, int mode, float param0, float param1,
                                  const ulcx_rate *d_rate, const float *d_pcm /* [n][nBlocks][BlockSize][nChan] */, int nBlocks,
                                  uint8_t *d_out /* [n][nBlocks][slot_bytes] */, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_encode_dev_pcm16_subset(ulcx_encoder *enc, const int32_t *d_slots, int n, int mode, float param0, float param1,
                                  const ulcx_rate *d_rate, const int16_t *d_pcm16, int nBlocks,
                                  uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_analyse_dev_subset     (ulcx_encoder *enc, const int32_t *d_slots, int n, const float *d_pcm, int nBlocks,
                                  int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_decode_dev_subset      (ulcx_decoder *dec, const int32_t *d_slots, int n, const uint8_t *d_in /* [n][nBlocks][slotBytes] */,
                                  int slotBytes, int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_dev_pcm16_subset(ulcx_decoder *dec, const int32_t *d_slots, int n, const uint8_t *d_in,
                                  int slotBytes, int nBlocks, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
/* Synchronous host forms (host pointers throughout; h_rate, when given, is validated as ulcx_encode_host_rates validates it).
 * Every check - list, record headers, rates - comes before any device work: a refused call leaves the object untouched. */
int  ulcx_encoder_reset_streams_host(ulcx_encoder *enc, const int32_t *h_slots, int n);
int  ulcx_encoder_save_streams_host (ulcx_encoder *enc, const int32_t *h_slots, int n, uint8_t *h_state);
int  ulcx_encoder_load_streams_host (ulcx_encoder *enc, const int32_t *h_slots, int n, const uint8_t *h_state);
int  ulcx_decoder_reset_streams_host(ulcx_decoder *dec, const int32_t *h_slots, int n);
int  ulcx_decoder_save_streams_host (ulcx_decoder *dec, const int32_t *h_slots, int n, uint8_t *h_state);
int  ulcx_decoder_load_streams_host (ulcx_decoder *dec, const int32_t *h_slots, int n, const uint8_t *h_state);
int  ulcx_encode_host_subset(ulcx_encoder *enc, const int32_t *h_slots, int n, int mode, float param0, float param1,
                             const ulcx_rate *h_rate, const float *h_pcm, int nBlocks,
                             uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx);
int  ulcx_decode_host_subset(ulcx_decoder *dec, const int32_t *h_slots, int n, const uint8_t *h_in, int slotBytes, int nBlocks,
                             float *h_pcm, int32_t *h_bits);
#define ULCX_STATE_MAGIC_ENC 0x45535855u      /* 'U' 'X' 'S' 'E' */
#define ULCX_STATE_MAGIC_DEC 0x44535855u      /* 'U' 'X' 'S' 'D' */

/* ------------------------------------------------------------------------- */
/* 3. `.ulc` container and packed streams               */
/* ------------------------------------------------------------------------- */
/* 24-byte little-endian file header, tools/ulc_Helper.h:10-20.  Blocks follow at
 * StreamOffs, each rounded up to a whole byte, with NO per-block length
 * (tools/ulcEncodeTool.c:160-169, tools/ulcDecodeTool.c:153-165). */
#define ULCX_ULC_MAGIC 0x32434C55u            /* 'U' | 'L'<<8 | 'C'<<16 | '2'<<24 */
typedef struct ulcx_file_header {
    uint32_t Magic;
    uint16_t BlockSize;
    uint16_t MaxBlockSize;                     /* largest block in bytes (0 = unknown) */
    uint32_t nBlocks;
    uint32_t RateHz;
    uint16_t nChan;
    uint16_t RateKbps;                         /* lrint(total_bytes*8*RateHz/1000/(BlockSize*nBlocks)), ulcEncodeTool.c:173-190 */
    uint32_t StreamOffs;
} ulcx_file_header;
void ulcx_ulc_header_pack(uint8_t dst[24], const ulcx_file_header *h);
int  ulcx_ulc_header_parse(ulcx_file_header *h, const uint8_t *src, size_t len);   /* 0 ok, ULCX_ERR_ARG: short / bad magic */
int  ulcx_ulc_rate_kbps(uint64_t totalBytes, uint32_t RateHz, uint32_t BlockSize, uint32_t nBlocks);

/* Concatenate the per-block slots an encode call produced into one contiguous payload
 * per stream (what the tool's fwrite loop produces).  Device pointers.
 *   d_payload      [nStreams][payloadStride] bytes, stream s starts at s*payloadStride
 *   d_payloadBytes [nStreams] bytes written;  d_maxBlock [nStreams] largest block (optional) */
int  ulcx_pack_streams_dev(int device, int nStreams, int nBlocks, int slotBytes, const uint8_t *d_slots, const int32_t *d_bits,
                           uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock, void *hipStream);

/* Decode the next nBlocks blocks of every stream from packed payloads: block k+1 begins at the
 * byte after block k ends, which only parsing reveals; the per-stream read position persists
 * across calls (ulcx_decoder_reset rewinds it).  d_payloadBytes[s] = valid bytes of stream s. */
int  ulcx_decode_packed_dev(ulcx_decoder *dec, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                            int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_packed_host(ulcx_decoder *dec, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                             int nBlocks, float *h_pcm, int32_t *h_bits);

/* Whole files (what ulcx-tool does, tools/ulcDecodeTool.c:123-166 batched): upload every stream's payload ONCE - the
 * read positions are rewound - then each ulcx_decode_resident_host call decodes the next nBlocks blocks of every stream
 * from the device-resident copy.  (ulcx_decode_packed_host uploads all payloads on every call.) */
int  ulcx_decoder_upload_payload(ulcx_decoder *dec, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes);
int  ulcx_decode_resident_host(ulcx_decoder *dec, int nBlocks, float *h_pcm, int32_t *h_bits);

/* Block index and seek: any block range of a packed stream without decoding what lies in front of it.
 * The container stores no block lengths, so a block's start is known only once every block in front of it has been
 * parsed.  The index is that walk done once, kept in a plain array the caller owns (it may be copied to the host, stored
 * beside the file and uploaded again later): per stream maxBlocks + 1 entries of 8 bytes.
 *   entry k, 0 <= k <= d_nBlocks[s]:  ByteOffs = byte of the stream's payload at which block k starts,
 *                                     RngState = state of the stream's noise generator there (ulcDecoder.c:75-81; the chain
 *                                     starts at 1234567, as every batched entry's does)
 *   entry d_nBlocks[s] closes the table: position and state behind the last whole block, so that the extent of block k is
 *   ByteOffs[k+1] - ByteOffs[k]; entries behind it are {-1, 0}.
 *   d_nBlocks[s] = whole, valid blocks found, at most maxBlocks: the walk stops where ulcx_decode_packed_dev would report
 *   0 bits (a corrupt block, the end of the payload).
 * maxBlocks is not limited by maxBlocksPerCall (the call uses none of the decoder's per-block scratch: a whole file is
 * indexed in one call).  The call reads the decoder's geometry and tables; it neither reads nor changes any stream's
 * state or read position.  Nothing outside [d_payload, d_payload + nStreams*payloadStride) is read.  Asynchronous on
 * hipStream; the _host form is synchronous. */
typedef struct ulcx_index_entry { int32_t ByteOffs; uint32_t RngState; } ulcx_index_entry;
int  ulcx_index_packed_dev(ulcx_decoder *dec, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                           int maxBlocks, ulcx_index_entry *d_index /* [nStreams][maxBlocks+1] */, int32_t *d_nBlocks /* [nStreams] */,
                           void *hipStream);
int  ulcx_index_packed_host(ulcx_decoder *dec, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                            int maxBlocks, ulcx_index_entry *h_index, int32_t *h_nBlocks);
/* Decode blocks d_first[s] .. d_first[s] + nBlocks - 1 of every stream s.
 *   d_index        [nStreams][indexStride] entries (indexStride = maxBlocks + 1 of the index call), d_indexBlocks [nStreams]
 *                  its block counts
 *   d_pcm          [nStreams][nBlocks][BlockSize][nChan], d_bits [nStreams][nBlocks]: bit for bit what a sequential decode from
 *                  block 0 writes for those blocks, the noise included
 * A block at or past d_indexBlocks[s] reports 0 bits and so does every later block of that stream in the call (as a
 * stream's end does in ulcx_decode_packed_dev); a d_first[s] outside [0, d_indexBlocks[s]] gives a stream of 0 bits (the
 * device forms cannot refuse it without a synchronisation; the host forms refuse a negative one with ULCX_ERR_ARG before
 * any device work).  Nothing outside the call's buffers is read or written.
 * A PAYLOAD THAT IS NOT THE ONE THE INDEX WAS BUILT FROM (bytes changed behind a stored index): every block is read at its index
 * offset and inside its index extent only.  A block that is corrupt, or that runs past its extent, ends the stream there for this
 * call - 0 bits and zero samples from it on, the blocks in front of it as they are; a corrupt block in front of the range gives
 * a stream of 0 bits.  A damaged block that still parses inside its extent is decoded as it reads, and behind it the noise follows
 * the draws actually made, counted from the stored RngState of the block in front of the range.  A stream none of whose blocks -
 * the block in front of the range included - is touched is unaffected.  The state left is the same continuation: a stream that
 * ended this way is dead for the packed calls that follow (a later range call does not inherit that), any other continues with the
 * block at the closing index entry of the range.  (tests/test_gpu_damaged_crops.py, against the reference decoder run block by block.)
 * After the call a stream's persistent state - lapping, LastSubBlockSize, generator, dead flag, packed read position - is
 * exactly what a sequential decode up to and including block d_first[s] + nBlocks - 1 leaves: a following
 * ulcx_decode_packed_dev on the same payload continues with the next block, and a later range call may go backwards.
 * nBlocks is 1 .. maxBlocksPerCall - 1: the block in front of a range is parsed and synthesised without output (its
 * lapping state is what the range's first block overlaps with) and takes one row of the call's per-block scratch. */
int  ulcx_decode_range_dev(ulcx_decoder *dec, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                           const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                           const int32_t *d_first /* [nStreams] */, int nBlocks,
                           float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_range_dev_pcm16(ulcx_decoder *dec, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                 const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                 const int32_t *d_first, int nBlocks,
                                 int16_t *d_pcm16 /* converted as ulcx_decode_dev_pcm16 converts */, int32_t *d_bits, void *hipStream);
int  ulcx_decode_range_host(ulcx_decoder *dec, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                            const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                            const int32_t *h_first, int nBlocks, float *h_pcm, int32_t *h_bits);   /* synchronous */
/* The same on the payload uploaded with ulcx_decoder_upload_payload: the index is built once and kept in the decoder
 * (h_nBlocks [nStreams], optional: the block counts), then any range is decoded from it.  A new upload drops the index. */
int  ulcx_decoder_index_resident(ulcx_decoder *dec, int maxBlocks, int32_t *h_nBlocks);
int  ulcx_decode_resident_range_host(ulcx_decoder *dec, const int32_t *h_first, int nBlocks, float *h_pcm, int32_t *h_bits);

/* Crops: row i of the call is blocks d_first[i] .. d_first[i] + nBlocks - 1 of file d_file[i] of a corpus of nFiles packed
 * payloads with their block indices.  nFiles is an argument of its own, not the decoder's nStreams (a 64-stream decoder
 * crops a corpus of 100 000 files); a file may be named by any number of rows, ranges may overlap or coincide.
 *   d_payload      [nFiles][payloadStride] bytes, d_payloadBytes [nFiles]; nFiles * payloadStride may exceed 2^31 (a single
 *                  file stays below 2^31 bytes: ByteOffs is an int32)
 *   d_index        [nFiles][indexStride] entries, d_indexBlocks [nFiles] their block counts (ulcx_index_packed_rows_dev, or
 *                  stored `.ulx` indices)
 *   n              rows of the call, 1 .. nStreams (the per-block scratch is the object's); nBlocks is 1 .. maxBlocksPerCall - 1,
 *                  as for a range call; nFiles >= 1
 *   d_file, d_first [n]; d_count [n] or NULL: the leading blocks wanted of each row, clamped to [0, nBlocks] - crops of
 *                  different length in one call
 *   d_pcm          [n][nBlocks][BlockSize][nChan], d_bits [n][nBlocks], written in full: row i is, bit for bit and with the noise
 *                  included, what a sequential decode of file d_file[i] from its block 0 writes for those blocks
 * A block at or past the file's d_indexBlocks, or at or past d_count[i], reports 0 bits and zero samples, and so does everything
 * behind it in the row.  The device forms cannot refuse a row without a synchronisation: a d_file[i] outside [0, nFiles), a
 * d_first[i] outside [0, d_indexBlocks[file]] and an index entry that points outside its file's payload each give a row of 0
 * bits and zero samples and leave the other rows as they are; nothing outside the call's buffers is read or written.  The host
 * form refuses a file number out of range, a first outside [0, h_indexBlocks[file]] and a negative count with ULCX_ERR_ARG
 * before any device work.
 * A file whose bytes changed behind its stored index is read as a range call reads it: each block inside its index extent; a block
 * that is corrupt or runs past its extent ends the row there (0 bits and zero samples from it on; a row whose block in front is such
 * a block is all zeros); behind a damaged block that still parses, the noise follows the draws actually made.  Rows none of whose
 * blocks, the block in front included, is touched - of the same file or of others - are unaffected.  The ragged and the sample
 * forms below do the same (a sample row is zero from the dead block's first sample to its exact end).
 * STATE: a crop call reads no stream's persistent state and changes none - lapping, LastSubBlockSize, generator, dead flag,
 * packed read position, resident payload, resident index.  It may be mixed freely with every other call on the object; a
 * sequential decode that is under way continues as if the crop call had not been made.  The call runs on the subset calls'
 * compact state copy (allocated on the first subset or crop call; nothing is allocated afterwards), and a refused call
 * leaves that copy as it was too.  ulcx_decoder_last_cut reports the call's launch plan, planned from n rows.
 * ALIGNMENT / EXTENT / ORDER as for every _dev call: d_file, d_first, d_count, d_payloadBytes, d_indexBlocks, d_index and d_bits
 * 4 bytes, d_pcm 16, d_pcm16 8, the payload none; a misaligned pointer returns ULCX_ERR_ARG before any device work.  Both
 * kernels go on hipStream and nothing waits for the device; the _host form is synchronous. */
int  ulcx_decode_crops_dev(ulcx_decoder *dec, int nFiles,
                           const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                           const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                           int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                           int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                 const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                 const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                 int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count,
                                 int nBlocks, int16_t *d_pcm16 /* converted as ulcx_decode_dev_pcm16 converts */, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_host(ulcx_decoder *dec, int nFiles,
                            const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                            const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                            int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                            int nBlocks, float *h_pcm, int32_t *h_bits);   /* synchronous */
/* ulcx_index_packed_dev with a row count of its own (the corpus's nFiles), as ulcx_index_slots_dev has one: entry for entry
 * what ulcx_index_packed_dev writes for the same payloads, for any nRows >= 1.  d_index [nRows][maxBlocks+1], d_nBlocks [nRows].
 * It reads the decoder's geometry and tables only. */
int  ulcx_index_packed_rows_dev(ulcx_decoder *dec, int nRows, const uint8_t *d_payload, long long payloadStride,
                                const int32_t *d_payloadBytes, int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream);
int  ulcx_index_packed_rows_host(ulcx_decoder *dec, int nRows, const uint8_t *h_payload, long long payloadStride,
                                 const int32_t *h_payloadBytes, int maxBlocks, ulcx_index_entry *h_index, int32_t *h_nBlocks);

/* Ragged corpus: the crop calls for files kept at their own length.  The strided layout above costs every file what the
 * longest one costs; here payloads and index rows lie back to back, found through two offset tables (CSR; caller-owned, plain
 * arrays):
 *   d_payload      payloadTotal bytes: the files' payloads back to back, no alignment; payloadTotal may be any size
 *   d_payloadOffs  int64 [nFiles + 1], 8-byte aligned: file f is bytes [offs[f], offs[f+1]) - its size is the difference, and stays
 *                  below 2^31
 *   d_index        indexTotal entries: the files' rows back to back
 *   d_indexOffs    int64 [nFiles + 1], 8-byte aligned, in entries: row f has capacity offs[f+1] - offs[f], and so at most
 *                  capacity - 1 blocks
 *   d_indexBlocks  [nFiles], as above
 * Everything else - n, nBlocks, d_file, d_first, d_count, rows past a file's end, STATE, ALIGNMENT / EXTENT / ORDER, the launch plan
 * ulcx_decoder_last_cut reports - is exactly as for ulcx_decode_crops_dev with the same file held in the strided layout, and so
 * is the output, bit for bit and with the noise included.
 * The tables are trusted as little as the strided walk trusts its own: a file number outside [0, nFiles), offs[f] < 0,
 * offs[f+1] < offs[f], offs[f+1] > the total, a file of 2^31 bytes or more, an index row whose capacity is below
 * d_indexBlocks[f] + 1 or that leaves [0, indexTotal], and an entry among those that bound the row's blocks that points outside
 * the file or not behind its predecessor each give a row of 0 bits and zero samples and leave the other rows as they are; no byte
 * outside [d_payload, d_payload + payloadTotal), the index and the call's buffers is read or written.  The host form refuses
 * with ULCX_ERR_ARG, before any device work, what ulcx_decode_crops_host refuses and an offset table that is not monotone or
 * leaves its buffer. */
int  ulcx_decode_crops_ragged_dev(ulcx_decoder *dec, int nFiles,
                                  const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                  const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                  const int32_t *d_indexBlocks /* [nFiles] */,
                                  int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                                  int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_ragged_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                        const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                        const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs,
                                        const int32_t *d_indexBlocks,
                                        int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count,
                                        int nBlocks, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_ragged_host(ulcx_decoder *dec, int nFiles,
                                   const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                   const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                   const int32_t *h_indexBlocks,
                                   int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                                   int nBlocks, float *h_pcm, int32_t *h_bits);   /* synchronous */
/* Sample crops: the crop calls with rows given in samples and the output written channels-first - what a training loader draws
 * (a crop of nSamples samples from sample t0 of a file) in the layout models take ([batch][channel][time]), straight from the
 * synthesis: the trim, the per-row offset and the planar layout happen where the samples are stored, no pass over the output.
 * The corpus arguments are those of ulcx_decode_crops_dev / ulcx_decode_crops_ragged_dev; n is 1 .. nStreams.
 *   d_start  int64 [n]: the row's first sample, a position in the DECODED stream of file d_file[i]: sample j of the stream is
 *            sample j % BlockSize of block j / BlockSize of the sequential decode.  The codec's delay is not compensated here
 *            (INTEGRATION.md section 2).
 *   d_len    [n] or NULL: samples wanted of the row, clamped to [0, nSamples]; NULL: nSamples for every row
 *   nSamples >= 1, any value (no multiple of anything); the blocks a row can touch, nB = ulcx_crop_blocks(BlockSize, nSamples),
 *            must be at most maxBlocksPerCall - 1
 *   d_pcm    [n][nChan][nSamples], written in full: d_pcm[i][ch][t] is, bit for bit and with the noise included, sample
 *            d_start[i] + t of channel ch of the sequential decode of the file, for t < d_len[i] and inside the file's whole
 *            valid blocks; zero everywhere else - behind d_len[i], behind the file's last indexed block, from a corrupt block on
 *   d_bits   [n][nB]: entry k is the size of block d_start[i] / BlockSize + k; 0 behind the blocks the row needs and behind the
 *            file's end - what a crop call with first = start / BlockSize and count = the blocks the row touches reports
 * Untrusted rows: whatever gives a crop row of zeros gives one here (a file number out of range, a bad index entry, bad ragged
 * tables), and so do d_start[i] < 0 and d_start[i] / BlockSize > d_indexBlocks[file]; the other rows are left alone and nothing
 * outside the call's buffers is read or written.  The host forms refuse, with ULCX_ERR_ARG before any device work, a negative
 * start, a start beyond the file's indexBlocks * BlockSize, a negative length, and whatever ulcx_decode_crops_host /
 * ulcx_decode_crops_ragged_host refuse.
 * STATE / ORDER: exactly the crop calls' - no stream's persistent state is read or changed, the call mixes freely with streaming
 * decodes on the object, it is asynchronous on hipStream (three kernels: the rows, the walk, the synthesis), and nothing is
 * allocated after the first subset or crop call.
 * ALIGNMENT: d_start 8 bytes; d_file, d_len, d_bits 4; d_pcm 4, d_pcm16 2 (a plane starts at any sample); the corpus as above. */
int  ulcx_crop_blocks(int BlockSize, int nSamples);   /* 1 + (nSamples + BlockSize - 2) / BlockSize: the blocks a crop touches at the worst start; host arithmetic (0: a bad argument) */
int  ulcx_decode_crops_samples_dev(ulcx_decoder *dec, int nFiles,
                                   const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                                   const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                                   int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                   int nSamples, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_samples_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                         const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                         const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                         int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                         int nSamples, int16_t *d_pcm16 /* converted as ulcx_decode_dev_pcm16 converts */, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_samples_host(ulcx_decoder *dec, int nFiles,
                                    const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                    const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                    int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                    int nSamples, float *h_pcm, int32_t *h_bits);   /* synchronous */
int  ulcx_decode_crops_samples_ragged_dev(ulcx_decoder *dec, int nFiles,
                                          const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                          const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                          const int32_t *d_indexBlocks /* [nFiles] */,
                                          int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                          int nSamples, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_samples_ragged_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                                const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs,
                                                const int32_t *d_indexBlocks,
                                                int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                                int nSamples, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_samples_ragged_host(ulcx_decoder *dec, int nFiles,
                                           const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                           const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                           const int32_t *h_indexBlocks,
                                           int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                           int nSamples, float *h_pcm, int32_t *h_bits);   /* synchronous */
/* Spectra: the crop calls stopped in front of the inverse transform - the dequantised MDCT coefficients of every block of a row,
 * the noise fill included, for models that take time-frequency input.  No FFT, no window, no lapping state and no synthesis of the
 * block in front of the range: behind the crop walk one workgroup per (row, block, channel pair) expands the walk's records.
 * The corpus, n, nBlocks, d_file, d_first and d_count are exactly the crop calls' (n is 1 .. nStreams, nBlocks is
 * 1 .. maxBlocksPerCall - 1, the walk's per-block scratch is the object's).  There is no PCM16 form: coefficients are not samples.
 *   d_coef  float32 [n][nChan][nBlocks][BlockSize], channels-first as the sample crops are: one channel's blocks form a
 *           [frames][bins] plane.  Written in full.  d_coef[i][ch][k] is, bit for bit and with the noise included, what the
 *           reference decoder holds in TransformBuffer for channel ch of block d_first[i] + k of a sequential decode of file
 *           d_file[i] from its block 0 (ulcDecoder.c:228-231): the block's sub-blocks in coded order, each S coefficients long.
 *           The values are the normalised coefficients of the CODED channels (mid / side for a pair); nothing is re-ordered onto
 *           a uniform grid, and the codec's delay is not compensated.
 *   d_wc    int32 [n][nBlocks]: the block's window code as the decoder forms it - the first nybble, | second << 4 when bit 3 is
 *           set, else | 0x10 - and 0 for a block that is not live.  ulcx_window_subblocks(BlockSize, wc, sizes) tells how the
 *           block's BlockSize coefficients split into shorter spectra.
 *   d_bits  int32 [n][nBlocks]: entry for entry what ulcx_decode_crops_dev writes for the same rows.  A block is live in this call
 *           exactly when it is live in the crop call, under every rule stated above for crops: a block past the file's end or past
 *           d_count, everything behind a corrupt block, a row whose block in front is corrupt, untrusted file numbers, firsts,
 *           index entries and ragged tables.  A block that is not live has 0 bits, wc 0 and coefficients of +0.0f.  Behind a
 *           damaged block that still parses, the noise follows the draws actually made, as in the crop call.
 *   flags   0, or ULCX_SPECTRA_LR: the channel pairs the decoder un-mixes in the time domain - (0,1), (2,3), ...; a trailing
 *           single channel is untouched (ulcDecoder.c:281-289) - come out as m + s and m - s, one float32 addition or subtraction
 *           per coefficient.  A block's window code is common to its channels and the transform is linear, so this is the
 *           linear-domain equivalent of the decoder's un-mixing: the spectrum of the left / right signal up to the rounding of
 *           the transform.  It is NOT a value the reference ever holds.  Any other bit: ULCX_ERR_ARG.
 * STATE / ORDER: the call reads and changes no stream's persistent state and mixes freely with every other call on the object
 * (it does not even touch the compact state copy the crop calls run on); it allocates nothing after the first subset or crop
 * call; the device forms are asynchronous on hipStream (two kernels: the walk, the expansion).  ulcx_decoder_last_cut reports
 * the plain plan (0 workgroups of a cut): the kernel's grid is n * nBlocks * ceil(nChan / 2) whatever n is.
 * The host forms refuse what ulcx_decode_crops_host / ulcx_decode_crops_ragged_host refuse, before any device work.
 * ALIGNMENT: d_coef 16 bytes; d_wc, d_bits, d_file, d_first, d_count and the corpus's int32 arrays 4; the ragged tables 8; a
 * misaligned pointer returns ULCX_ERR_ARG before any device work. */
#define ULCX_SPECTRA_LR 1   /* flags: left/right instead of the coded mid/side (see above) */
int  ulcx_window_subblocks(int BlockSize, int wc, int sizes[4]);
    /* host arithmetic: the number of sub-blocks (1..4) of a block with window code wc and their sizes in coded order (unused
       entries 0; sizes may be NULL); 0 for a code no block can carry - among them 0, a block that is not live - or a bad
       BlockSize.  A decimated header whose second nybble is 0 or 1 (no row of FormatSpecs.md's table; the reference decodes it
       as one full-size block) gives 1 sub-block of BlockSize. */
int  ulcx_decode_crops_spectra_dev(ulcx_decoder *dec, int nFiles,
                                   const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                                   const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                                   int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                                   int nBlocks, int flags, float *d_coef, int32_t *d_wc, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_spectra_host(ulcx_decoder *dec, int nFiles,
                                    const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                    const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                    int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                                    int nBlocks, int flags, float *h_coef, int32_t *h_wc, int32_t *h_bits);   /* synchronous */
int  ulcx_decode_crops_spectra_ragged_dev(ulcx_decoder *dec, int nFiles,
                                          const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                          const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                          const int32_t *d_indexBlocks /* [nFiles] */,
                                          int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                                          int nBlocks, int flags, float *d_coef, int32_t *d_wc, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_spectra_ragged_host(ulcx_decoder *dec, int nFiles,
                                           const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                           const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                           const int32_t *h_indexBlocks,
                                           int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                                           int nBlocks, int flags, float *h_coef, int32_t *h_wc, int32_t *h_bits);   /* synchronous */
/* Distortion: the spectra calls with the coded planes summed on chip against caller-held reference planes instead of written - how
 * good a coded file is, per (row, channel, block, segment of the spectrum), without a coded plane in HBM.  The reference is
 * typically the clean spectrum of the same clip on the same grid (ulcx_analyse_clips_* / ulcx_encode_clips_spectra_*, section 2);
 * with no reference the call is a band-energy extractor of the coded corpus.  The corpus, n, d_file, d_first, d_count, nBlocks,
 * d_wc, d_bits and hipStream are exactly the spectra calls'; in place of d_coef:
 *   d_ref      float32 [nRef][nChan][nRefBlocks][BlockSize], laid out as the spectra calls' d_coef, or NULL: no reference (nRef,
 *              nRefBlocks, d_refRow and d_refFirst are then ignored).  Taken as it is: under ULCX_SPECTRA_LR pass planes made with it.
 *   d_refRow   int32 [n], optional: the reference row of crop row i (NULL: i).  Several rows may name one reference row.
 *   d_refFirst int32 [n], optional: the reference block paired with output block 0 of row i (NULL: 0).
 *   nSeg       segments per block: a power of two, 1 .. 64, with BlockSize / nSeg >= 4.  Segment g covers coefficients
 *              [g * W, (g + 1) * W), W = BlockSize / nSeg, in CODED order, as the planes are.  Sub-block boundaries of a decimated
 *              block are multiples of BlockSize / 8: from nSeg >= 8 on every segment lies inside one sub-block.
 *   flags      0 or ULCX_SPECTRA_LR, with the spectra calls' meaning.
 *   d_dist     binary64 [n][nChan][nBlocks][nSeg][3] = {S, Y, E}, written in full.  With y[j] the value
 *              ulcx_decode_crops_spectra_dev writes at d_coef[i][ch][k][j] under the same flags, and
 *              r[j] = d_ref[d_refRow[i]][ch][d_refFirst[i] + k][j]:   S = sum r^2,  Y = sum y^2,  E = sum (r - y)^2  over the segment.
 * ARITHMETIC, which is the contract: every term is formed in binary64 from the float32 values - (double)r * (double)r and
 * (double)y * (double)y (exact), d = (double)r - (double)y (one subtraction), d * d (one multiplication); no contraction; float32
 * denormals are values, not zeros.  The W terms of a segment are added by the pairwise tree over adjacent elements: level 0 is the
 * terms, t[l+1][j] = t[l][2j] + t[l][2j+1].  So every result is one defined bit pattern, and the result at nSeg is the pairwise sum
 * of the results at 2 * nSeg, down to the whole block.
 * ABSENT REFERENCE: d_ref NULL, a d_refRow[i] outside [0, nRef), or a reference block d_refFirst[i] + k (formed in 64 bits) outside
 * [0, nRefBlocks) make that block's reference all +0.0f, and nothing is read for it: S = 0 and E = Y.  Both tables are untrusted,
 * as d_file is.
 * LIVENESS: d_wc and d_bits are entry for entry the spectra call's, under every rule stated for it.  A block that is not live has
 * +0.0 in all three sums of every segment, and its reference is not read.  NaN / Inf in the reference stay inside their segment.
 * STATE / ORDER: the spectra calls' - no stream's persistent state is read or changed, nothing is allocated after the first subset
 * or crop call, the device forms are asynchronous on hipStream (two kernels: the walk, the reduction; the grid is the spectra
 * call's).  ULCX_ERR_ARG before any device work for: whatever the spectra call refuses; a bad nSeg; d_dist NULL or not 8-byte
 * aligned; d_ref not 16-byte aligned; d_ref != NULL with nRef < 1 or nRefBlocks < 1; d_refRow / d_refFirst not 4-byte aligned; a
 * flag other than ULCX_SPECTRA_LR; and ULCX_SPECTRA_LR at a BlockSize whose two unit arrays do not fit a compute unit's LDS
 * (32768): left and right cannot be formed on chip there without a plane to park the first channel in.  The mid/side form works
 * at every BlockSize.  The host forms are synchronous and refuse what the spectra host forms refuse. */
int  ulcx_decode_crops_distortion_dev(ulcx_decoder *dec, int nFiles,
                                      const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                                      const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                                      int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                                      int nBlocks, const float *d_ref /* optional */, int nRef, int nRefBlocks,
                                      const int32_t *d_refRow /* optional */, const int32_t *d_refFirst /* optional */, int nSeg, int flags,
                                      double *d_dist, int32_t *d_wc, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_distortion_host(ulcx_decoder *dec, int nFiles,
                                       const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                       const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                       int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                                       int nBlocks, const float *h_ref, int nRef, int nRefBlocks,
                                       const int32_t *h_refRow, const int32_t *h_refFirst, int nSeg, int flags,
                                       double *h_dist, int32_t *h_wc, int32_t *h_bits);   /* synchronous */
int  ulcx_decode_crops_distortion_ragged_dev(ulcx_decoder *dec, int nFiles,
                                             const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                             const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                             const int32_t *d_indexBlocks /* [nFiles] */,
                                             int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count /* optional */,
                                             int nBlocks, const float *d_ref /* optional */, int nRef, int nRefBlocks,
                                             const int32_t *d_refRow /* optional */, const int32_t *d_refFirst /* optional */, int nSeg, int flags,
                                             double *d_dist, int32_t *d_wc, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_distortion_ragged_host(ulcx_decoder *dec, int nFiles,
                                              const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                              const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                              const int32_t *h_indexBlocks,
                                              int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                                              int nBlocks, const float *h_ref, int nRef, int nRefBlocks,
                                              const int32_t *h_refRow, const int32_t *h_refFirst, int nSeg, int flags,
                                              double *h_dist, int32_t *h_wc, int32_t *h_bits);   /* synchronous */
/* Synthesis from spectra: the way back - PCM from caller-held MDCT planes, through the decoder's own inverse transform (pre-twiddle,
 * FFT, post-twiddle with the windowed overlap, the centring of decimated sub-blocks, lapping state), the very kernels the crop
 * calls run, with the syntax walk replaced by loads from the planes.  For models that work on the planes of the spectra calls or
 * of the clip-spectra calls (section 2) and have to be heard and scored in the time domain.
 *   d_coef  float32 [n][nChan][nBlocks][BlockSize], d_wc int32 [n][nBlocks]: layout, sub-block order and window-code convention are
 *           exactly what ulcx_decode_crops_spectra_*, ulcx_analyse_clips_* and ulcx_encode_clips_spectra_* write - their outputs go
 *           in unchanged.  THE WINDOW CODES MUST ACCOMPANY THE PLANES: they say how a plane splits into sub-blocks and which
 *           window overlaps them.  n is 1 .. nStreams.
 *   flags   ULCX_SYNTH_WARM: plane 0 of every row is the block in FRONT of the output: it is transformed for the lapping state
 *           and the LastSubBlockSize it leaves, and has no output.  nOut = nBlocks - (WARM ? 1 : 0) is 1 .. maxBlocksPerCall - 1
 *           (the call uses the object's per-block scratch rows, as the crop calls do).
 *           ULCX_SPECTRA_LR: the planes already hold left/right, and the time-domain un-mix (ulcDecoder.c:281-289) is skipped.
 *           Without it the pairs (0,1), (2,3), ... are un-mixed as the decoder does it; a trailing single channel is left alone.
 *           Any other bit: ULCX_ERR_ARG.
 *   d_pcm   [n][nChan][nOut * BlockSize], channels-first as the sample crops are, written in full.  Output block k of row i is,
 *           bit for bit, what a freshly initialised reference decoder (LastSubBlockSize 0, TransformInvLap zero) writes that holds
 *           the row's planes in TransformBuffer and d_wc[i][k] in WindowCtrl, block after block, from ulcDecoder.c:217 on.  The
 *           PCM16 form rounds as every PCM16 form does (lrintf of the clamped sample * 2^15).
 *           The PCM of a block depends on the planes and codes of that block and the one in front only.  Hence
 *           ulcx_decode_crops_spectra_dev(first - 1, nBlocks + 1), then this call with ULCX_SYNTH_WARM, is bit for bit
 *           ulcx_decode_crops_samples_dev of nBlocks whole blocks from block `first`; without WARM the same holds for rows with
 *           first = 0.  Without WARM on planes from mid-stream only output block 0 differs (it laps against silence).
 *           d_pcm must not overlap d_coef (not checked).
 *   d_live  int32 [n][nOut]: 1 where the block was synthesised, 0 where it was not.  A row ends at its first plane whose code
 *           fails ulcx_window_subblocks(BlockSize, wc, NULL) > 0 - 0, the spectra calls' "not live", and any int32 no block can
 *           carry: that block and everything behind it come out as +0.0 samples and live 0, as a corrupt block ends a decode; a
 *           bad plane in front (WARM) ends the whole row.  Other rows are untouched.  d_wc is not trusted: it is validated on the
 *           device before it steers anything.  Coefficient VALUES are not inspected: NaN and Inf travel through the arithmetic
 *           and cannot leave the two blocks and the row they belong to.
 * STATE / ORDER: the call reads and changes no stream's persistent state (it runs on the compact state copy of the subset and crop
 * calls) and mixes freely with every other call on the object; it allocates nothing after the first subset or crop call; the
 * device forms are asynchronous on hipStream (two kernels: the rows' prologue, the synthesis).  The launch plan is the range
 * call's for the same n and nOut: few long rows are cut evenly, a workgroup that enters a row mid-way runs the plane in front
 * without output; ulcx_decoder_last_cut reports it.
 * ALIGNMENT: d_coef and d_pcm 16 bytes; d_pcm16, d_wc and d_live 4; a misaligned or NULL pointer returns ULCX_ERR_ARG before any
 * device work. */
#define ULCX_SYNTH_WARM 2   /* flags: plane 0 of every row is the block in front of the output (see above) */
int  ulcx_synth_spectra_dev(ulcx_decoder *dec, int n, int nBlocks, int flags, const float *d_coef, const int32_t *d_wc,
                            float *d_pcm, int32_t *d_live, void *hipStream);
int  ulcx_synth_spectra_dev_pcm16(ulcx_decoder *dec, int n, int nBlocks, int flags, const float *d_coef, const int32_t *d_wc,
                                  int16_t *d_pcm16, int32_t *d_live, void *hipStream);
int  ulcx_synth_spectra_host(ulcx_decoder *dec, int n, int nBlocks, int flags, const float *h_coef, const int32_t *h_wc,
                             float *h_pcm, int32_t *h_live);   /* synchronous */
/* The index of a ragged corpus in one call: row f receives, entry for entry, what ulcx_index_packed_rows_dev writes for file f's
 * payload alone with maxBlocks = capacity - 1, the {-1, 0} entries behind the closing one up to the row's capacity included, and
 * d_nBlocks[f] the count.  A row of capacity below 1, or a file whose offsets are as refused above, gets d_nBlocks[f] = 0 and no
 * entry; nothing outside [d_indexOffs[f], d_indexOffs[f+1]) is written for file f.  It reads the decoder's geometry and tables
 * only, and no stream state.  One lane walks one file, so files of very different length in one wave wait for the longest.
 * The host form refuses an offset table that is not monotone or leaves its buffer; entries of h_index outside the rows stay. */
int  ulcx_index_packed_ragged_dev(ulcx_decoder *dec, int nFiles, const uint8_t *d_payload, long long payloadTotal,
                                  const int64_t *d_payloadOffs, ulcx_index_entry *d_index, long long indexTotal,
                                  const int64_t *d_indexOffs, int32_t *d_nBlocks, void *hipStream);
int  ulcx_index_packed_ragged_host(ulcx_decoder *dec, int nFiles, const uint8_t *h_payload, long long payloadTotal,
                                   const int64_t *h_payloadOffs, ulcx_index_entry *h_index, long long indexTotal,
                                   const int64_t *h_indexOffs, int32_t *h_nBlocks);

/* Index while encoding: the same table, grown call by call from what an encode call wrote - every block in its own slot,
 * its size in d_bits - so all of a call's blocks are parsed side by side and nothing is walked in series.  The result is,
 * entry for entry, what ulcx_index_packed_dev builds from the same blocks after ulcx_pack_streams_dev.
 * The decoder object supplies the geometry (nChan, BlockSize) and the tables only: nRows is an argument of its own, not the
 * decoder's nStreams (a one-stream decoder indexes 4096 rows; the [n] rows of a subset call; a ladder call's
 * [nRungs][nStreams] output as nRungs * nStreams rows in one call).  No stream state is read or changed, none of the
 * per-block scratch is used (nBlocks is not limited by maxBlocksPerCall) and nothing is allocated.
 *   ulcx_index_begin_dev  opens nRows rows: entry 0 = {0, 1234567}, entries 1 .. indexStride-1 = {-1, 0}, d_nBlocks[s] = 0.
 *   ulcx_index_slots_dev  appends.  Row s, with n0 = d_nBlocks[s] on entry: m = the leading blocks k of the row for which
 *       d_bits[k] > 0 and d_bits[k] / 8 <= slotBytes; the walk of slot k, limited to d_bits[k] bits, is valid and consumes
 *       (bits + 7) / 8 == d_bits[k] / 8 bytes; n0 + k + 1 <= indexStride - 1; and the new ByteOffs fits in an int32.
 *       Entries n0+1 .. n0+m receive the running byte offset and the generator state (continued from entry n0's), entries
 *       n0+m+1 .. min(n0 + nBlocks, indexStride - 1) are written {-1, 0}, d_nBlocks[s] = n0 + m.  A row whose n0 is outside
 *       [0, indexStride - 1] is left untouched, count included.  A stream that is shorter in a call (d_bits 0 from some
 *       block on) stops growing there; a later call appends behind it.
 *   d_slots [nRows][nBlocks][slotBytes], d_bits [nRows][nBlocks] (multiples of 8, as the encoder writes them),
 *   d_index [nRows][indexStride], d_nBlocks [nRows].  ALIGNMENT / EXTENT / ORDER as for every _dev call.
 * The _host form is synchronous (h_index and h_nBlocks are read and written); it refuses an h_nBlocks entry outside
 * [0, indexStride - 1] with ULCX_ERR_ARG before any device work. */
int  ulcx_index_begin_dev(ulcx_decoder *dec, int nRows, ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, void *hipStream);
int  ulcx_index_slots_dev(ulcx_decoder *dec, int nRows, const uint8_t *d_slots, int slotBytes, const int32_t *d_bits, int nBlocks,
                          ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, void *hipStream);
int  ulcx_index_slots_host(ulcx_decoder *dec, int nRows, const uint8_t *h_slots, int slotBytes, const int32_t *h_bits, int nBlocks,
                           ulcx_index_entry *h_index, int indexStride, int32_t *h_nBlocks);
/* Host code, no GPU: is `row` (indexStride entries, nBlocks of them blocks) an index a range call may be given for a payload
 * of payloadBytes?  Entry 0 = {0, 1234567}, ByteOffs strictly increasing over entries 0 .. nBlocks, the closing offset
 * <= payloadBytes, 0 <= nBlocks < indexStride.  Returns 0 or ULCX_ERR_ARG. */
int  ulcx_index_check(const ulcx_index_entry *row, int nBlocks, int indexStride, long long payloadBytes);
/* A stored index for the payload uploaded with ulcx_decoder_upload_payload, in place of ulcx_decoder_index_resident (no walk):
 * h_index [nStreams][indexStride], h_nBlocks [nStreams].  Every row must pass ulcx_index_check against its stream's uploaded
 * payload size (ULCX_ERR_ARG otherwise: the decoder is as it was, an index it had included).  A new upload drops the index. */
int  ulcx_decoder_set_resident_index(ulcx_decoder *dec, const ulcx_index_entry *h_index, int indexStride, const int32_t *h_nBlocks);

/* Clips: the encode mirror of the sample-crop calls.  Row i of the call is a whole clip in samples, channels-first, at its own
 * length, encoded from a fresh state; the call's output is a resident corpus - payloads, byte counts, block index, block counts -
 * that ulcx_decode_crops_* and ulcx_decode_crops_samples_* read the moment the call returns on the stream.
 *   n        rows, 1 .. nStreams of the encoder;  nSamples >= 1: samples per plane of d_pcm, any value
 *   d_pcm    [n][nChan][nSamples] binary32 (d_pcm16: int16, converted on load as ulcx_encode_dev_pcm16 converts); row i is the clip
 *            d_pcm[i][ch][0 .. L_i), L_i = d_len[i] clamped to [0, nSamples], d_len NULL: nSamples
 *   mode / param0 / param1, or d_rate [n] in the tool's convention: exactly as ulcx_encode_dev_subset takes them
 *   dec      supplies geometry and tables for the index, as for ulcx_index_slots_dev (same device, nChan and BlockSize as enc;
 *            its nStreams and maxBlocksPerCall do not matter)
 * A row with L_i >= 1 gets nb_i = ulcx_clip_blocks(BlockSize, L_i) blocks: what ULC_EncodeBlock_* of a freshly created encoder
 * writes under the row's setting for the clip, interleaved, then zeros - the blocks of the `.ulc` file the tool writes for that
 * clip alone (tools/ulcEncodeTool.c:93-98,133-169).  d_payload[i * payloadStride ..] holds them back to back, d_payloadBytes[i]
 * their length, d_maxBlock[i] (optional) the largest block.  Row i of d_index ([n][indexStride]) and d_indexBlocks[i] are, entry
 * for entry, what ulcx_index_packed_rows_dev builds from that payload with maxBlocks = indexStride - 1, the {-1, 0} entries
 * behind the closing one included.  A row with L_i == 0 is empty: 0 bytes, 0 blocks, the open index row.
 * CAPACITY.  A row keeps its leading whole blocks that fit payloadStride and indexStride - 1 and stops growing there (the rule of
 * ulcx_index_slots_dev for a stream that stops); d_indexBlocks[i] < ulcx_clip_blocks(BlockSize, L_i) tells a truncated row.
 * payloadStride >= ulcx_encoder_slot_bytes * ulcx_clip_blocks(BlockSize, nSamples) always suffices.
 * STATE.  The call reads and changes no slot of enc and no stream state of dec: it runs the plain call's launch sequence on the
 * subset calls' shadow state, reset to the state right after create, and scatters nothing back.  It mixes freely with streaming,
 * subset, ladder and analysis calls on the object; a refused call leaves everything as it was.  The staging of the call (one chunk
 * of interleaved input, slots and sizes) is the object's, allocated on the first clips call; nothing is allocated afterwards (but by a clips
 * ladder call of more rungs, below).
 * ORDER.  Everything is enqueued on hipStream and nothing waits for the device: ceil(ulcx_clip_blocks(BlockSize, nSamples) /
 * maxBlocksPerCall) chunks of (stage, the launch sequence, append, index).  Rows that have ended go on encoding silence that is
 * masked; the encoder is causal in its input, so the chunking changes no byte.
 * The _dev forms refuse with ULCX_ERR_ARG before any device work: a NULL required pointer, a misaligned one (d_pcm 4 bytes,
 * d_pcm16 2, d_rate 8, everything else 4, the payload none), nSamples < 1, indexStride < 2, payloadStride < 1, a bad scalar mode
 * without a table, n outside 1 .. nStreams, a decoder of another geometry or device.  The host form is synchronous; it knows the
 * lengths, refuses a negative h_len entry and a bad rate entry too, and stops at the longest row's last chunk. */
int  ulcx_clip_blocks(int BlockSize, int nSamples);   /* (nSamples + BlockSize - 1) / BlockSize + 2 for nSamples >= 1; 0 for nSamples <= 0 or a bad BlockSize; host arithmetic */
int  ulcx_encode_clips_dev(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *d_rate /* [n] or NULL */,
                           const float *d_pcm /* [n][nChan][nSamples] */, const int32_t *d_len /* [n] or NULL */, int nSamples,
                           uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes /* [n] */, int32_t *d_maxBlock /* [n], optional */,
                           ulcx_index_entry *d_index /* [n][indexStride] */, int indexStride, int32_t *d_indexBlocks /* [n] */, void *hipStream);
int  ulcx_encode_clips_dev_pcm16(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *d_rate,
                                 const int16_t *d_pcm16, const int32_t *d_len, int nSamples,
                                 uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock,
                                 ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, void *hipStream);
int  ulcx_encode_clips_host(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *h_rate,
                            const float *h_pcm, const int32_t *h_len, int nSamples,
                            uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes, int32_t *h_maxBlock,
                            ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks);   /* synchronous */

/* Clips ladder: the clips call under nRungs rate settings in ONE call - the same clip at several rates, two-pass ABR included.
 * Rows (d_pcm / d_pcm16, d_len, nSamples, ulcx_clip_blocks) and dec are exactly the clips call's; rungs are ulcx_rung as
 * ulcx_encode_dev_ladder takes them with nStreams read as n (a table rung: a DEVICE table [n]; a host table in the host form).
 * Staging, window control, transform, complexity, Bark levels and noise spectrum run once per chunk, selection and writer once
 * per rung (the ladder's launch sequence on the shadow state), then one append and one index launch over all files.
 * OUTPUT.  One corpus of nRungs * n files: file r * n + i is clip i under rung r - its payload at d_payload + (r * n + i) *
 * payloadStride, its index row d_index[r * n + i], its counts at [r * n + i] of d_payloadBytes / d_maxBlock / d_indexBlocks.  The
 * crop calls take it as it is (nFiles = nRungs * n, d_file = r * n + i).  Every file is byte for byte and entry for entry what
 * ulcx_encode_clips_dev writes for that clip under rung r's setting; with one rung without AUTO the call writes what the plain
 * clips call writes.
 * CAPACITY.  The clips call's rule per FILE: rung r of row i keeps its leading whole blocks that fit payloadStride and
 * indexStride - 1, whatever the other rungs of that row keep (a high-rate rung may stop blocks before a low-rate one).
 * ULCX_RUNG_AUTO in ulcx_rung::reserved - the tool's `RATE,auto` (cli/ulcx_tool.c; tools/ulcEncodeTool.c:130,164,178).  In front of
 * the encode ONE analysis pass over all chunks runs (the launch sequence of ulcx_analyse_clips_* on the freshly reset shadow
 * state), shared by every AUTO rung; it gives row i  avg_i = (float)(S_i / nb_i),  nb_i = ulcx_clip_blocks(BlockSize, L_i),  S_i
 * the binary64 sum of the row's BlockComplexity values added in block order 0 .. nb_i - 1 - all of the clip's blocks, whatever
 * the capacities keep.  An AUTO rung then encodes row i at {RateKbps, avg_i}: RateKbps is param0 of a scalar rung (mode CBR or
 * ABR, param0 finite and > 0; param1 is ignored) or the row's entry of a table rung (the table's own AvgComplexity is ignored;
 * a row with RateKbps < 0 stays the VBR row it is).  avg_i == 0 means CBR, as the table convention has it.  The caller's tables
 * are not written: the resolved tables [ULCX_MAX_RUNGS][nStreams] live in the object.  An AUTO scalar rung therefore behaves
 * as a table rung (always the full number of probe passes).  A call without an AUTO rung runs no analysis pass.
 *   d_avg   optional, float32 [n]: avg_i (0 for an empty row).  WITHOUT an AUTO rung it is NOT written.
 * STATE / ORDER.  The clips call's rules: no slot of enc and no stream state of dec is read or changed, everything is enqueued on
 * hipStream, nothing waits for the device; the shadow state is reset in front of the analysis pass and again in front of the
 * encode pass; the call mixes freely with every other call on the object.  STAGING: the object's slots and sizes of a chunk hold
 * nRungs rungs - nRungs * nStreams * maxBlocksPerCall * slot_bytes bytes of slots - and grow to the largest clips ladder seen
 * (the rule of ulcx_encode_host_ladder's staging; growing allocates the larger staging, then frees the smaller one, which waits for
 * the device; if the allocation fails the call returns ULCX_ERR_NOMEM and the object keeps the staging it had): size
 * maxBlocksPerCall by it.  After the call ulcx_encoder_last_rungs is nRungs.
 * The _dev forms refuse with ULCX_ERR_ARG before any device work, the object as it was: everything the clips call refuses;
 * everything ulcx_encode_dev_ladder refuses except `reserved`; `reserved` outside {0, ULCX_RUNG_AUTO}; AUTO on a scalar rung of
 * mode VBR or with a param0 that is no rate; a rung table not aligned to 8 bytes, d_avg not aligned to 4; nRungs * n * indexStride
 * beyond what ulcx_index_slots_dev takes.  The host form is synchronous (h_payload .. h_indexBlocks hold nRungs * n files); it
 * also refuses a bad table entry and bad scalar parameters as ulcx_encode_host_ladder does, and AUTO on a table row with
 * RateKbps < 0.  ulcx_encode_*_ladder go on refusing any non-zero `reserved`. */
#define ULCX_RUNG_AUTO 1   /* in ulcx_rung::reserved, accepted by the clips ladder calls only */
int  ulcx_encode_clips_ladder_dev(ulcx_encoder *enc, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                  const float *d_pcm /* [n][nChan][nSamples] */, const int32_t *d_len /* [n] or NULL */, int nSamples,
                                  uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes /* [nRungs][n] */, int32_t *d_maxBlock /* [nRungs][n], optional */,
                                  ulcx_index_entry *d_index /* [nRungs][n][indexStride] */, int indexStride, int32_t *d_indexBlocks /* [nRungs][n] */,
                                  float *d_avg /* [n], optional */, void *hipStream);
int  ulcx_encode_clips_ladder_dev_pcm16(ulcx_encoder *enc, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                        const int16_t *d_pcm16, const int32_t *d_len, int nSamples,
                                        uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock,
                                        ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, float *d_avg, void *hipStream);
int  ulcx_encode_clips_ladder_host(ulcx_encoder *enc, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                   const float *h_pcm, const int32_t *h_len, int nSamples,
                                   uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes, int32_t *h_maxBlock,
                                   ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks, float *h_avg);   /* synchronous */

/* Clip spectra: the encoder's own MDCT coefficients of clips - the encode mirror of ulcx_decode_crops_spectra_*, and with it the
 * clean half of a (coded spectrum, clean spectrum) pair on one grid: the same layout, under the window code the encoder chose for
 * that very block.  Two families on the clips calls' rows (d_pcm / d_pcm16 [n][nChan][nSamples], d_len, nSamples: exactly as above,
 * every row from a fresh state):
 *   ulcx_analyse_clips_*         no rate, no decoder, no corpus: per chunk the analysis launch sequence of ulcx_analyse_dev (window
 *                                control, the MDCT-only transform, the ordered sums)
 *   ulcx_encode_clips_spectra_*  ulcx_encode_clips_* with the tap: the arguments of the clips call, then nBlocks .. d_cplx.  The
 *                                corpus it writes is byte for byte and entry for entry the plain clips call's; window control and
 *                                the transform run once for both outputs.
 *   nBlocks  >= 1: the depth of the caller's planes, any value; ulcx_clip_blocks(BlockSize, nSamples) holds every row in full.
 *            Block k of row i is LIVE when k < min(nBlocks, ulcx_clip_blocks(BlockSize, L_i)), L_i the clamped length.  Liveness
 *            depends on the length alone, not on payloadStride / indexStride: a row truncated by capacity still has all its
 *            spectra, and d_indexBlocks[i] tells how many of them have a coded partner.
 *   d_coef   float32 [n][nChan][nBlocks][BlockSize], channels-first as the decode side's; required; written in full.  A live block
 *            holds, bit for bit, what the reference encoder holds in TransformBuffer for channel ch after ULC_EncodeBlock_* of
 *            block k of that clip (interleaved, then zeros) from a freshly created encoder: the normalised coefficients of the
 *            mid / side channels, the block's sub-blocks in coded order.  A block that is not live is +0.0f, the planes behind the
 *            call's last chunk included.
 *   d_wc     optional, int32 [n][nBlocks]: State->WindowCtrl of the block, 0 where the block is not live.  This is the value
 *            ulcx_decode_crops_spectra_* reports for that block of the encoded file - an un-decimated block: 0x10 | the overlap
 *            scale; a decimated one: the low nybble with bit 3 set, the pattern in the high nybble - so
 *            ulcx_window_subblocks(BlockSize, wc, sizes) splits both sides' blocks alike.
 *   d_cplx   optional, float32 [n][nBlocks]: State->BlockComplexity after the block, +0.0f where the block is not live.
 *   flags    0, or ULCX_SPECTRA_LR with the decode side's meaning: pairs (0,1), (2,3), ... come out as m + s and m - s, one
 *            float32 addition or subtraction per coefficient, a trailing single channel untouched.  NOT a value the reference
 *            holds.  Any other bit: ULCX_ERR_ARG.
 * PAIRING.  ulcx_encode_clips_spectra_dev, then ulcx_decode_crops_spectra_dev on the corpus it wrote with d_file[i] = i and
 * d_first[i] = 0 (a decoder of maxBlocksPerCall > nBlocks): block k of row i of the two d_coef arrays is the clean and the coded
 * spectrum of the same block, and the two d_wc arrays agree, for every k < d_indexBlocks[i].
 * STATE / ORDER: the clips call's rules.  No slot of enc is read or changed; everything is enqueued on hipStream and nothing
 * waits for the device; the chunks are the clips call's, each followed by one more kernel (one workgroup per row, block and
 * channel pair), and plane blocks behind the last chunk are zeroed by a last launch of it.  The staging of a chunk's window
 * codes and complexities is the object's, allocated on the first such call; nothing is allocated afterwards.  After an analysis
 * form the object is as ulcx_analyse_dev leaves it (ulcx_encoder_debug_fetch refuses, ulcx_encoder_last_rungs is 0), after an
 * encode form as the clips call leaves it.
 * The _dev forms refuse with ULCX_ERR_ARG before any device work what the clips call refuses (the analysis forms: without the
 * rate, corpus and decoder checks), and: d_coef NULL or not aligned to 16 bytes, d_wc / d_cplx not aligned to 4, nBlocks < 1, a
 * bad flag.  The host forms are synchronous, refuse what ulcx_encode_clips_host refuses, and stop at the longest row's last chunk. */
int  ulcx_analyse_clips_dev(ulcx_encoder *enc, int n, const float *d_pcm /* [n][nChan][nSamples] */, const int32_t *d_len /* [n] or NULL */, int nSamples,
                            int nBlocks, int flags, float *d_coef /* [n][nChan][nBlocks][BlockSize] */, int32_t *d_wc /* [n][nBlocks], optional */,
                            float *d_cplx /* [n][nBlocks], optional */, void *hipStream);
int  ulcx_analyse_clips_dev_pcm16(ulcx_encoder *enc, int n, const int16_t *d_pcm16, const int32_t *d_len, int nSamples,
                                  int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_analyse_clips_host(ulcx_encoder *enc, int n, const float *h_pcm, const int32_t *h_len, int nSamples,
                             int nBlocks, int flags, float *h_coef, int32_t *h_wc, float *h_cplx);   /* synchronous */
int  ulcx_encode_clips_spectra_dev(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *d_rate,
                                   const float *d_pcm, const int32_t *d_len, int nSamples,
                                   uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock,
                                   ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks,
                                   int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_encode_clips_spectra_dev_pcm16(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *d_rate,
                                         const int16_t *d_pcm16, const int32_t *d_len, int nSamples,
                                         uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock,
                                         ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks,
                                         int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream);
int  ulcx_encode_clips_spectra_host(ulcx_encoder *enc, ulcx_decoder *dec, int n, int mode, float param0, float param1, const ulcx_rate *h_rate,
                                    const float *h_pcm, const int32_t *h_len, int nSamples,
                                    uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes, int32_t *h_maxBlock,
                                    ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks,
                                    int nBlocks, int flags, float *h_coef, int32_t *h_wc, float *h_cplx);   /* synchronous */

/* Strided corpus -> ragged corpus on the device: the layout ulcx_decode_crops_ragged_* and ulcx_decode_crops_samples_ragged_* read,
 * from the strided one (a clip call's output, or any corpus held for ulcx_decode_crops_dev).  No object: `device` is the HIP ordinal.
 * File f contributes clamp(d_payloadBytes[f], 0, payloadStride) bytes and clamp(d_indexBlocks[f], 0, indexStride - 1) + 1 entries
 * (its row up to and including the closing entry); d_payloadOffs / d_indexOffs [nFiles + 1] are the exclusive int64 prefix sums,
 * d_outIndexBlocks [nFiles] the clamped counts.  The files are laid out in order while both running totals stay within payloadCap
 * bytes and indexCap entries: the capacities of d_outPayload and d_outIndex.  The ragged crop calls read nothing outside
 * [d_payload, d_payload + payloadTotal) and so ask for no slack behind the last payload: payloadCap needs none either (a
 * caller who wants the 64 bytes corpus.py leaves passes a cap that much below its buffer).  The first file that does not fit,
 * and every file behind it, gets an empty range in both tables and 0 blocks - the crop calls give rows of zeros for it.
 * d_need [2] always receives the bytes and the entries the WHOLE corpus needs, so that a caller can allocate and call again.
 * payloadTotal / indexTotal for the crop calls: the capacities, or d_payloadOffs[nFiles] / d_indexOffs[nFiles].
 * Asynchronous on hipStream (two kernels); ULCX_ERR_ARG before any device work for nFiles < 1, a stride below 1, a negative
 * capacity, a NULL or misaligned pointer (offset tables and d_need 8 bytes, counts and index 4, payloads none). */
int  ulcx_corpus_ragged_dev(int device, int nFiles,
                            const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes, const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                            uint8_t *d_outPayload, long long payloadCap, int64_t *d_payloadOffs /* [nFiles+1] */,
                            ulcx_index_entry *d_outIndex, long long indexCap, int64_t *d_indexOffs /* [nFiles+1] */, int32_t *d_outIndexBlocks /* [nFiles] */,
                            int64_t *d_need /* [2]: bytes and entries the whole corpus needs */, void *hipStream);
int  ulcx_corpus_ragged_host(int device, int nFiles,
                             const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes, const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                             uint8_t *h_outPayload, long long payloadCap, int64_t *h_payloadOffs,
                             ulcx_index_entry *h_outIndex, long long indexCap, int64_t *h_indexOffs, int32_t *h_outIndexBlocks,
                             int64_t *h_need);   /* synchronous */

/* Corpus splice: new files made of block ranges of resident files - rung switches of a ladder corpus, trims, joins.  The source
 * is a strided corpus as ulcx_decode_crops_dev takes it (or a ragged one, as ulcx_decode_crops_ragged_dev does); the output is a
 * strided corpus exactly as a clip call leaves one: every crop call reads it the moment the call returns on hipStream, and
 * ulcx_corpus_ragged_dev converts it.  `dec` supplies geometry and tables only, as for ulcx_index_slots_dev: nFiles, nOut and
 * nSeg are the call's own (limited neither by nStreams nor by maxBlocksPerCall), no stream state is read or changed, none of the
 * object's per-block scratch is used, nothing is allocated, and the call mixes freely with every other call on the object.
 *
 * Positions are whole blocks.  Blocks are byte-aligned and self-contained, so a splice is a byte copy plus a new block index:
 * the generator state in front of a block depends on the draws of the blocks now in front of it, and is rebuilt from a parse of
 * every block taken (the source index's RngState is never read).
 *
 * Output file o is the segments d_segOffs[o] .. d_segOffs[o + 1] - 1 of d_seg, in order (CSR).  It takes the blocks they name one
 * by one and stops growing at the first block that cannot be taken - which may lie in the middle of a segment; everything behind
 * it is absent (the rule of a stream that stops in ulcx_index_slots_dev).  Block k of source file f can be taken when
 *   - File is in [0, nFiles), First >= 0, and k < clamp(d_indexBlocks[f], 0, indexStride - 1) (ragged: the file's offsets and row
 *     capacity are ones the ragged crop calls accept);
 *   - 0 <= ByteOffs[k] < ByteOffs[k + 1] <= the file's byte count;
 *   - the parse of those bytes, limited to that extent, is valid and consumes exactly the extent: a block damaged behind a stored
 *     index ends the output file in front of it;
 *   - it fits: the running block count stays within outIndexStride - 1, the running byte count within outPayloadStride and an int32.
 * A segment whose Count is 0 or negative names no block and contributes nothing.  A file with no segment, or whose first block
 * cannot be taken, is empty: 0 bytes, 0 blocks, the open index row.  An output file whose d_segOffs pair falls or leaves
 * [0, nSeg] is empty, and those of its segments that exist get d_segStart = -1.
 *
 * Written: d_outPayload[o * outPayloadStride ..] the taken blocks back to back (bytes behind d_outPayloadBytes[o] are not
 * written); row o of d_outIndex and d_outIndexBlocks[o], entry for entry what ulcx_index_packed_rows_dev builds from that payload
 * with maxBlocks = outIndexStride - 1, the {-1, 0} entries behind the closing one included; d_outMaxBlock[o] (optional) the
 * largest taken block in bytes; d_segStart[j] the output block at which segment j begins in the plan - the sum of max(Count, 0)
 * over the earlier segments of its output file, saturating at INT32_MAX - whatever is taken: segment j is present in full exactly
 * when d_segStart[j] + Count <= d_outIndexBlocks[o].  It is an output for labels that follow their blocks, and the table the
 * kernels search: required.
 *
 * The _dev forms enqueue everything on hipStream and wait for nothing; ULCX_ERR_ARG before any device work for a NULL required
 * pointer, a misaligned one (offset tables 8 bytes, every other table 4, payloads none), nFiles / nOut / nSeg below 1, a stride
 * below 1 (ragged: a negative total), outIndexStride < 2, more output than one call's grids take, or an output payload or index
 * range that overlaps the source's payload or index.  The host forms are synchronous and know the tables: they also refuse an
 * h_segOffs that does not rise from >= 0 to <= nSeg, a File out of range, a negative First or Count, First + Count beyond
 * h_indexBlocks[File], and (ragged) what ulcx_decode_crops_ragged_host refuses of the offset tables. */
typedef struct ulcx_segment { int32_t File, First, Count; } ulcx_segment;   /* blocks First .. First + Count - 1 of source file File; 12 bytes */
int  ulcx_corpus_splice_dev(ulcx_decoder *dec, int nFiles,
                            const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                            const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                            int nOut, const int32_t *d_segOffs /* [nOut+1] */, const ulcx_segment *d_seg, int nSeg,
                            uint8_t *d_outPayload, long long outPayloadStride, int32_t *d_outPayloadBytes /* [nOut] */, int32_t *d_outMaxBlock /* [nOut], optional */,
                            ulcx_index_entry *d_outIndex, int outIndexStride, int32_t *d_outIndexBlocks /* [nOut] */,
                            int32_t *d_segStart /* [nSeg] */, void *hipStream);
int  ulcx_corpus_splice_ragged_dev(ulcx_decoder *dec, int nFiles,
                                   const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                   const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                   int nOut, const int32_t *d_segOffs, const ulcx_segment *d_seg, int nSeg,
                                   uint8_t *d_outPayload, long long outPayloadStride, int32_t *d_outPayloadBytes, int32_t *d_outMaxBlock,
                                   ulcx_index_entry *d_outIndex, int outIndexStride, int32_t *d_outIndexBlocks,
                                   int32_t *d_segStart, void *hipStream);
int  ulcx_corpus_splice_host(ulcx_decoder *dec, int nFiles,
                             const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                             const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                             int nOut, const int32_t *h_segOffs, const ulcx_segment *h_seg, int nSeg,
                             uint8_t *h_outPayload, long long outPayloadStride, int32_t *h_outPayloadBytes, int32_t *h_outMaxBlock,
                             ulcx_index_entry *h_outIndex, int outIndexStride, int32_t *h_outIndexBlocks,
                             int32_t *h_segStart);   /* synchronous; of h_outPayload only bytes [0, h_outPayloadBytes[o]) of each file are written */
int  ulcx_corpus_splice_ragged_host(ulcx_decoder *dec, int nFiles,
                                    const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                    const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                    int nOut, const int32_t *h_segOffs, const ulcx_segment *h_seg, int nSeg,
                                    uint8_t *h_outPayload, long long outPayloadStride, int32_t *h_outPayloadBytes, int32_t *h_outMaxBlock,
                                    ulcx_index_entry *h_outIndex, int outIndexStride, int32_t *h_outIndexBlocks,
                                    int32_t *h_segStart);   /* synchronous */

/* `.ulx` sidecar: the block index of ONE `.ulc` file, written beside it (stem.ulx).  16-byte little-endian header, then
 * nBlocks + 1 entries of 8 bytes (ByteOffs, RngState; offsets relative to the .ulc file's StreamOffs).  The `.ulc` container
 * itself stays the reference's. */
#define ULCX_ULX_MAGIC 0x31584C55u            /* 'U' | 'L'<<8 | 'X'<<16 | '1'<<24 */
#define ULCX_ULX_HEADER_BYTES 16
typedef struct ulcx_index_file_header {
    uint32_t Magic;
    uint16_t BlockSize;
    uint16_t nChan;
    uint32_t nBlocks;                          /* blocks indexed: nBlocks + 1 entries follow */
    uint32_t PayloadBytes;                     /* size of the .ulc file's payload the index was made for */
} ulcx_index_file_header;
void ulcx_ulx_header_pack(uint8_t dst[16], const ulcx_index_file_header *h);
int  ulcx_ulx_header_parse(ulcx_index_file_header *h, const uint8_t *src, size_t len);   /* 0 ok, ULCX_ERR_ARG: short / bad magic */

/* Timing helper for bench.py: device time (ms, hipEvent) of the kernels the last
 * ulcx_*_dev call enqueued, per pipeline stage; returns number of stages written.
 * Only valid after the stream has been synchronised. */
int  ulcx_encoder_stage_ms(ulcx_encoder *enc, float *ms, int maxStages);
/* The events behind the two calls above are recorded around every kernel of every ulcx_*_dev call (default on);
 * a caller that never reads them can switch them off. */
int  ulcx_encoder_set_timing(ulcx_encoder *enc, int on);
int  ulcx_decoder_set_timing(ulcx_decoder *dec, int on);
const char *ulcx_encoder_stage_name(int stage);
/* Launches of the transform kernel (k_xf) in the last call: the stage time above is their sum (1 when the
 * window-control pipeline is off). */
int  ulcx_encoder_last_xf_launches(ulcx_encoder *enc);
int  ulcx_decoder_stage_ms(ulcx_decoder *dec, float *ms, int maxStages);
const char *ulcx_decoder_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif
