// ulcx_internal.h — structures shared by the host API (ulcx_api.cpp) and the HIP
// kernels (ulcx_enc.hip / ulcx_dec.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ulc_amd.h"

#ifndef ULCX_DSYN_TWL
#define ULCX_DSYN_TWL 1                  // stereo synthesis, BlockSize <= 2048: FFT twiddles in LDS (0: from the tables in global memory; A/B builds)
#endif
#define ULCX_NBARK 25
#define ULCX_MAX_SUB 4
#define ULCX_BARK_EVENTS 52              // 25 lower edges + 25 upper edges + end of subblock (+ pad)
#define ULCX_MAX_BS_DEVICE 32768       // the reference's own limit (ulcEncoder.c:32-34); above 8192 the transform takes one array at a time (k_xf_big)
#define ULCX_COEF_EPS (0x1.0p-31f)     // include/ulcEncoder.h:36
#define ULCX_HEAP_LDS_BYTES (128 * 1024)
#define ULCX_HEAP_GRID 256
#define ULCX_DONE_VBR 2                  // cbrDone of a VBR block in a per-stream-rates call (any non-zero value means "no search left")
// Ablation switches for timing experiments (they break the results): compiled in only with `make EXTRA=-DULCX_ABLATE`,
// then set by ULCX_DBG_SKIP=bits at create time.  The shipped library has no such branches.
#ifdef ULCX_ABLATE
#define ULCX_DBG(c) ((c).dbgSkip)
#else
#define ULCX_DBG(c) 0
#endif

// Host-precomputed, data-independent tables: everything
// the reference evaluates with sinhf/asinhf/cos/sin or expf on arguments that depend
// only on (BlockSize, RateHz).  Built with the HOST libm in ulcx_tables.cpp, one
// set per encoder/decoder, resident in HBM (hot in L2).  Index d = log2(BS/S).
struct UlcxTables {
    const float2 *pre[ULCX_MAX_SUB];     // DCT-IV pre/post twiddle P[n] = (cos,sin)(pi(8n+1)/(8S)), n < S/2
    const float2 *tw[ULCX_MAX_SUB];      // FFT twiddle W[j] = (cos,sin)(2 pi j / (S/2)), j < S/4
    const float  *winFall;               // ramp for overlap Ov (power of two) at [Ov + i], i < Ov
    const float  *winRise;
    const int    *bandIdx[ULCX_MAX_SUB]; // per line < S/2: (int)Bark(line)         Psyopt.c:141-143,237-239
    const float  *bandFrac[ULCX_MAX_SUB];//               Bark(line) - (int)Bark(line)
    const float4 *bandW[ULCX_MAX_SUB];   // the two above ready to use (round 6): per line {index of the left Bark level, of the right one - both
                                         // clamped as Psyopt.c:143-147 / :240-244 clamp them, as int bits -, 1 - frac, frac}
    const uint32_t *barkSched;           // [2][ULCX_MAX_SUB][ULCX_BARK_EVENTS] band edges in line order (k_bark_uniform)
    // Bark band edges per subblock size (lines of the S/2-line pseudo-DFT)
    short nBeg[ULCX_MAX_SUB][ULCX_NBARK], nEnd[ULCX_MAX_SUB][ULCX_NBARK];   // noise:  [b, b+2)        Psyopt.c:198-205
    short pBeg[ULCX_MAX_SUB][ULCX_NBARK], pEnd[ULCX_MAX_SUB][ULCX_NBARK];   // psycho: [b-.75, b+.25)  Psyopt.c:109-116
};

struct UlcxWcState {                     // per stream, persistent (ulcEncoder.h:65-77)
    float tf[3];                         // TransientFilter
    int   wcPrev, wcCur;                 // WindowCtrl of block k0-1 and k0 (k0 = next call's first block)
    float binSum[8], binW[8];            // TransientBuffer R half of the last analysed block
    int   pad;
};

struct UlcxEncCtx {
    // geometry
    int B, K, C, BS, lgBS;               // streams, blocks this call, channels, block size
    int barkRing;                        // k_bark_uniform: snapshots a lane keeps of open Bark bands (power of two; 0 = k_nbark / k_pbark for every block)
    int *decList, *decCount;             // blocks of this call with a decimated window (listed by the transform): they take k_nbark / k_pbark
    int maxK;                            // allocation stride for per-call arrays
    int slot;                            // bytes per output slot
    int unitCap;                         // bytes per (chan,subblock) nybble staging row = 2*BS+32 per channel
    int mode; float p0, p1;              // rate control
    float vbrTarget;                     // 0x1.E4EFB7p3f*logf(100/Quality) (host libm), ulcEncoder.c:144
    const float2 *rates;                 // [B] per-stream {RateKbps, AvgComplexity} (ulcx_encode_*_rates: replaces mode/p0/p1); NULL = the scalar setting
    // window-control constants (1 - rate), host expf: WindowControl.c:75,76,94,95,120
    float cHP, cBP, qHP, qBP, cBlk;
    float cplxScale;                     // BlockTransform.c:320
    int   rateHz;
    UlcxTables T;
    // inputs / outputs of this call
    int keyFinal;                        // c.key holds this call's final keys (k_keys_finalize has run): consumers read them instead of forming them
    const float *pcm; const int16_t *pcm16;      // exactly one is set: the C API's f32 input, or PCM16 ingest
    uint8_t *out; int32_t *bits; int32_t *wcOut; float *cplxOut;
    // persistent state
    float *hist;                         // [B][2*BS][C] previous two input blocks (raw, interleaved)
    UlcxWcState *wcs;                    // [B]
    // per-call scratch
    float2 *env;                         // [ceil(B/64)][maxK*BS][64] {hp,bp} energies -> envelopes -> transient curve (.x)
    float  *bins;                        // [B][maxK+1][16] {Sum[8],SumW[8]}; row 0 = previous block
    int    *wcArr;                       // [B][maxK+2] WindowCtrl of blocks k0-1 .. k0+K
    float  *coef;                        // [NB][C*BS]   normalised MDCT (TransformBuffer)
    float  *key;                         // [NB][C*BS]   key0 = FastLog(Re^2) | -inf; final keys are formed on the fly (final_key)
    float  *nsum;                        // [NB][C*BS/2] per-line |X|^2 (noise input)
    float  *npair;                       // [NB][C*BS]   {w, w*log} pairs (TransformNoise): parity tap only, allocated on its first use
    float  *amp2;                        // [NB][BS/2]
    float  *barkN;                       // [NB][C*4][25]
    float  *barkP;                       // [NB][4][25]
    double *barkRawN, *barkRawP;         // [rows][25][3] ordered sums of each band of un-decimated blocks (k_bark_uniform -> k_bark_levels)
    int    *nnz;                         // [NB]
    float  *cplx;                        // [NB]
    int    *nout;                        // [NB]   nOutCoef of the current pass
    int    *cbrLo, *cbrHi, *cbrDone;     // [NB]  (cbrDone = ULCX_DONE_VBR: a VBR block of a per-stream-rates call - no search, nOut = nTargetCoef)
    uint32_t *keep;                      // [NB][C*BS/32]
    int    *fbList; int *fbCount;        // tie-straddle fallback list
    uint8_t *unitBuf;                    // [NB][C][unitCap]
    int    *unitNyb;                     // [NB][C*4]
    int    *cbrBudget;                   // [NB] bit budget (ulcEncoder.c:96)
    uint4  *selWin;                      // [NB] rate search: {TL, TH, count(key >= TL), count(key >= TH)} - the ordered-key window later probes search
    uint32_t *selT;                      // [NB] the threshold key of the current probe
    int     selPair;                     // stereo BlockSize 4096: the selection with a wave per channel (k_select_pair); ULCX_SEL_PAIR=0: one wave per block
    int     selPass;                     // k_select_wave in a rate search: 1 = first probe (stores the ordered keys in `key`), 2 = later ones (read them); 0 = one-pass call
    int    *cbrLive;                     // [1] rate searches of the lock-step path still open (probe passes leave at once at 0)
    int    *slow;                        // [NB] wave-encoder give-up bits (1: small caps, 2: full caps -> k_encode_units); then 2 queue counters, 2 retry queues [NB]
    float2 *gapSum;                      // [NB][C*BS] {Sum, SumW} of the noise run in front of each kept coefficient (speculative)
    float  *tailSum;                     // [NB][C*4][8] five HF-extension sums + start index of the tail they assume
    int     useGapSums;
    int    *isFb;                        // [NB] 1 = a threshold tie group straddled the cut this call: block is on the exact (rank) path
    int    *ownSlot;                     // [NB] its slot in fbList
    int    *rankBuf;                     // [rankSlots][C*BS] full heapsort ranking of exact-path blocks
    int     dbgSkip;
    int     forceFb;                     // test hook (ulcx_encoder_debug_force_exact): every forceFb-th block takes the exact path whatever its ties
    int     rankSlots, fbLo, fbHi;       // resident rank slots; slot window of the current exact-path launch
    int     fbMode;                      // 0 = all blocks, 1 = skip isFb blocks, 2 = only isFb blocks
    int     useWave;                     // wave-per-unit encode pass (k_encode_wave); serial kernel only for overflow blocks
    int     directPack;                  // the wave writer packs stereo un-decimated blocks into the output slot itself (ULCX_DIRECT_PACK=0: k_pack does all)
    void   *heapScratch;                 // [ULCX_HEAP_GRID][C*BS] {key,idx} heaps, only when C*BS*8 exceeds the LDS budget
};

struct UlcxDecCtx {
    int B, K, C, BS, lgBS, maxK;
    int s0, s1;                          // streams [s0, s1) this launch works on
    int slot;
    int dbgSkip;                         // timing experiments only (ULCX_DBG_SKIP)
    UlcxTables T;
    const uint8_t *in; float *pcm; int16_t *pcm16;   // exactly one of pcm / pcm16 is set (f32 as the C API, or PCM16 output)
    long long inBytes;                   // readable extent of `in`: nothing outside [in, in + inBytes) is touched
    int32_t *bits;
    // persistent
    float *lap;                          // [B][C][BS/2] TransformInvLap
    int   *lastSub;                      // [B] LastSubBlockSize
    uint32_t *seed;                      // [B] noise RNG state (ulcDecoder.c:75-81)
    int   *dead;                         // [B] stream hit a corrupt block
    // k_dsyn with several workgroups per stream (round 3): the state after the launch goes to a second set of arrays (a
    // workgroup that enters a stream in the middle reads the state in front of the launch while the one that finishes the
    // stream writes the new one); the host swaps the two sets afterwards.  Without a split both sets are the same arrays.
    float *lapO; int *lastSubO; uint32_t *seedO; int *deadO;
    float *lapScratch;                   // [cut workgroups][C][BS/2] a workgroup's own lapping state between its blocks
    int    synFull;                      // cut launches: the first synFull workgroups take one whole stream each, the rest an even cut of the remaining streams
    int    k0, k1;                       // blocks [k0, k1) of every stream this synthesis launch works on
    // per-call scratch: what the scan leaves for the synthesis (ulcx_dec.hip)
    int   *wcScan;                       // [NB] WindowCtrl as the scan saw it (0 = corrupt)
    int   *draws;                        // [NB] RNG draws consumed by the block
    int   *unitDraws;                    // [NB][C*4] draws made in the block before each (chan,subblock) unit
    float4 *unitTail;                    // [NB][C*4] decaying-noise tail of the unit: {start level, decay, first coefficient, count}
    int4  *unitRec;                      // [NB][C*4] {first plain-run record, count, first noise record, count} of the unit
    uint2 *prec; int precStride;         // [NB][C*BS] plain-run records of the block (ulcx_dec.hip scan_block)
    uint2 *nrec; int nrecStride;         // [NB][C*BS/16 + C*4] noise records
    float *tailMag;                      // [NB][C*4][tailStride] tail level at every 32nd coefficient of the unit
    int    tailStride;                   // BS/32
    float *scratch;                      // [B][4*BS] general-path staging of time samples (decimated / non-stereo blocks)
    const uint32_t *jumpT;               // [8][16][4][256] byte tables of T^(d*16^i), T = one xorshift32 step
    const uint32_t *parT;                // [4][256][64] byte tables, lane fastest: a lane's word of a unit's sign-parity stream from the unit's start state
    int    fastOK, twInLds;              // stereo fast path / its FFT twiddles resident in LDS (0 or 1)
    // packed-stream mode (.ulc payloads): blocks are located by parsing, not by slot
    int   packed;
    long long payStride;                 // bytes between stream payloads
    const int32_t *payBytes;             // [B] valid bytes per stream
    int  *packOff;                       // [B] persistent read position of each stream
    int  *blkOff;                        // [NB] byte offset of each block inside its stream payload
    // range calls (ulcx_decode_range_*): blocks rFirst[s] .. rFirst[s] + K - 2 of every stream, found through a block index.
    // A stream has K = nBlocks + 1 rows of the per-block scratch: row 0 is the block in front of the range (run without
    // output, for the lapping state), rows 1 .. K-1 the blocks of the call; the synthesis works on rows [k0 = 1, K).
    int   range;
    const ulcx_index_entry *rIndex;      // [B][rIndexStride]
    int   rIndexStride;
    const int32_t *rIndexBlocks, *rFirst;   // [B] entries of each stream's index that are blocks; first block of the range
    int2 *rInfo;                         // [B] {1 = row 0 holds a block, generator state in front of the stream's first row} (k_dscan_rows)
    int32_t *bitsOut;                    // [B][K-1] the caller's sizes (c.bits: the rows' own, [B][K])
};

// ulcHelper.h:24-46
__host__ __device__ static inline unsigned ulcx_pattern(int wc) {
    // (ulcHelper.h:24-46, the sixteen patterns packed four to a 64-bit constant and picked by selects and a shift: as a switch
    //  this became a table in constant memory - a scalar load with its wait at the top of every workgroup of the transform,
    //  a 64-address gather in the lane-per-block kernels)
    const unsigned i = ((unsigned)wc >> 4) & 15u;
    const unsigned long long t0 = 0x0091001900080000ull, t1 = 0x0A2102A101A2012Aull, t2 = 0x1B3213B212B3123Bull, t3 = 0xB3213B212B3123B1ull;
    const unsigned long long t = (i & 8u) ? ((i & 4u) ? t3 : t2) : ((i & 4u) ? t1 : t0);
    return (unsigned)(t >> (16u * (i & 3u))) & 0xFFFFu;
}

// host side (ulcx_tables.cpp)
int  ulcx_tables_build(UlcxTables *devT, void **devBlob, int BS, int rateHz, bool forEncoder);
int  ulcx_tables_bark_ring(const UlcxTables &T, int BS, int *mostOpen);   // the snapshot ring of k_bark_uniform for full-size band tables (0: none fits); the most bands open at one line
void ulcx_set_error(const char *fmt, ...);

// launchers (ulcx_enc.hip / ulcx_dec.hip)
#define ULCX_ENC_STAGES 20
#define ULCX_ENC_STAGES_REPORTED (ULCX_ENC_STAGES + 1)   // + "wc_pipeline_exposed" (computed, not an event interval)
extern const char *const ulcx_enc_stage_names[ULCX_ENC_STAGES_REPORTED];
#define ULCX_DEC_STAGES 2
#define ULCX_WC_MAXCH 32    // fine steps of the window-control pipeline per call
#define ULCX_XF_MAXCH 8     // coarse transform chunks per call
#define ULCX_LDS_LIMIT (160 * 1024)     // LDS per workgroup on gfx950
// Streams (all three, or none: everything on the caller's) and events of the encoder launch, one event per role; the untimed ones first: created and destroyed as an array.
struct UlcxEncSync {
    hipEvent_t wcStart, wcForward[ULCX_WC_MAXCH], wcBackward[ULCX_WC_MAXCH], wcDecided[ULCX_WC_MAXCH];   // window-control pipeline: caller's -> side, then per fine step side -> side2 -> side3 -> caller's
    hipEvent_t xfChunkDone[ULCX_XF_MAXCH], cplxChunksDone;   // transform chunk j done: its k_cplx may start on side; every chunk's k_cplx done
    hipEvent_t noiseFork, noiseDone, tailFork, tailDone;     // side2: noise log-spectrum behind the transform, joined in front of the writer; k_tails beside k_nsums
    hipEvent_t cplxDone, stateDone;      // side3: k_cplx, joined in front of the selection; k_state_update, joined at the end of the call
    hipEvent_t exactFork, exactFork2, exactJoin;             // exact path on side: behind the selection, behind the noise join, back
    hipEvent_t xfTiming[2 * ULCX_XF_MAXCH];                  // timed: pairs around each transform launch of a pipelined call (recorded when ev != NULL)
    hipStream_t side, side2, side3;
};
struct UlcxEncAux {                      // what a call's launch needs beside its UlcxEncCtx (filled by enc_aux, ulcx_api.cpp)
    UlcxEncSync &sync;
    int wcPipe;                          // chunks of blocks pipelined between window control and transform; 1 = off (> 1 only with side streams)
    int wcSteps, wcFuse, nsSlots;        // fine window-control steps per call (ULCX_WC_STEPS); stereo: k_wc_ef; resident workgroups of k_nsums (its persistent grid)
    int &nXf;                            // out: transform launches of a pipelined call (0: one launch, no xfTiming pairs)
};
// Where a call of K blocks is cut: nCh transform chunks [cut[j], cut[j + 1]) beside nW window-control steps [wcs[w], wcs[w + 1]).
// nCh <= 1: the plain launch, one range of each (nW = 1).  Host arithmetic only; launch_front (ulcx_enc.hip) launches by it and
// ulcx_encoder_debug_front_plan (ulcx_api.cpp) reports it.
struct UlcxFrontPlan { int nCh, nW; int cut[ULCX_XF_MAXCH + 1]; int wcs[ULCX_WC_MAXCH + 1]; };
static inline UlcxFrontPlan ulcx_front_plan(int K, int wcPipe, int wcSteps) {
    UlcxFrontPlan p;
    p.nCh = wcPipe;
    if (p.nCh <= 1) { p.nCh = 1; p.nW = 1; p.cut[0] = p.wcs[0] = 0; p.cut[1] = p.wcs[1] = K; return p; }
    // The window-control kernels advance in uniform steps of a few blocks (ULCX_WC_STEPS; 0 = in the same chunks as
    // the transform: first chunk one block, then thirds).  Measured with the chunked transform: 4 steps 8.65-8.70 ms
    // per step of 65536 blocks, 8 steps 8.73-8.81, 16 steps 8.9-9.0 (every launch of a chain kernel costs its fixed
    // latency, and a step that has to be dispatched beside a transform chunk waits for its workgroup slots).
    int nW = wcSteps;
    if (nW < 0) nW = (K >= 8) ? 4 : 0;                                 // default: 4 uniform steps (of >= 2 blocks)
    if (nW > ULCX_WC_MAXCH) nW = ULCX_WC_MAXCH;
    if (nW > K) nW = K;
    const bool sameCuts = nW < 1;
    if (sameCuts) nW = p.nCh;
    // (transform chunks cut where the window-control steps end - eight blocks behind the first step instead of one - :
    //  the transform's interval +0.37 ms, the exposed window control -0.37 ms, the phase the same 4.0 ms)
    p.cut[0] = 0; p.cut[1] = 1;
    for (int j = 2; j <= p.nCh; j++) p.cut[j] = 1 + (K - 1) * (j - 1) / (p.nCh - 1);
    for (int w = 0; w <= nW; w++) p.wcs[w] = sameCuts ? p.cut[w] : (int)((long long)K * w / nW);
    p.nW = nW;
    return p;
}
int ulcx_enc_launch(const UlcxEncCtx &c, hipStream_t st, hipEvent_t *ev /* ULCX_ENC_STAGES+1 or NULL */, const UlcxEncAux &aux);
// ulcx_encode_*_ladder: one context per rung (rung 0's carries wcOut / cplxOut); k_rung_arm arms rungs >= 1 (ulcx_enc_ladder.hip)
int ulcx_enc_launch_ladder(const UlcxEncCtx *rungs, int nRungs, hipStream_t st, hipEvent_t *ev, const UlcxEncAux &aux);
void ulcx_enc_rung_arm(const UlcxEncCtx &c, hipStream_t st);
// A corpus of indexed files in HBM, strided or ragged (payOffs != NULL): the one description every call family that finds a file
// and a block in a corpus hands its kernels, by value - crops, sample crops, spectra, splice, and a range call, whose corpus is
// the decoder's own streams (file = stream).  corpus_file / file_block (ulcx_dec_dev.h) are the one reading of it; none of its
// tables is trusted.  Pointers are device pointers in a launch, host pointers while a host form checks and uploads them.
struct UlcxCorpus {
    const uint8_t *pay; long long payTotal;                  // the whole payload buffer: nothing outside it is read
    const ulcx_index_entry *index; long long idxTotal;      // the whole index, in entries
    const int32_t *indexBlocks;          // [nFiles] entries of each file's row that are blocks
    int nFiles;
    int ragged;                          // host side only: the entry is a ragged form (its tables may still be NULL, and are then refused)
    // strided: file f is payBytes[f] bytes at pay + f * payStride, its row the indexStride entries at index + f * indexStride
    long long payStride; const int32_t *payBytes; int indexStride;
    // ragged: file f is bytes [payOffs[f], payOffs[f + 1]) of pay, its row the entries [idxOffs[f], idxOffs[f + 1]) of index
    const int64_t *payOffs, *idxOffs;    // [nFiles + 1]
};
static inline UlcxCorpus ulcx_corpus_strided(int nFiles, const uint8_t *pay, long long payStride, const int32_t *payBytes, const ulcx_index_entry *index,
                                             int indexStride, const int32_t *indexBlocks) {
    return UlcxCorpus{ pay, (long long)nFiles * payStride, index, (long long)nFiles * indexStride, indexBlocks, nFiles, 0, payStride, payBytes, indexStride, nullptr, nullptr };
}
static inline UlcxCorpus ulcx_corpus_ragged(int nFiles, const uint8_t *pay, long long payTotal, const int64_t *payOffs, const ulcx_index_entry *index,
                                            long long idxTotal, const int64_t *idxOffs, const int32_t *indexBlocks) {
    return UlcxCorpus{ pay, payTotal, index, idxTotal, indexBlocks, nFiles, 1, 0, nullptr, 0, payOffs, idxOffs };
}
// The blocks of an index row of `entries` entries that counts nI, as every walk reads a count: the closing entry stays inside the
// row.  (The kernels' file view and the host forms' row checks both call this.)
__host__ __device__ static inline long long ulcx_row_blocks(long long nI, long long entries) { return nI < 0 ? 0 : nI > entries - 1 ? entries - 1 : nI; }

// What kind of call a decode launch serves: set where the API layer knows it, read by dec_launch (ulcx_api.cpp) and ulcx_dec_launch.
// Everything from RANGE on is a range launch (c.range = 1): rows entered from nothing through a block index.
enum UlcxDecKind {
    ULCX_DEC_PLAIN,                      // slots or packed payloads, from and to the streams' state: no aux field is looked at
    ULCX_DEC_RANGE,                      // ulcx_decode_range_*: the decoder's own streams as a strided corpus (file = stream), c.rIndex* / c.rFirst
    ULCX_DEC_CROPS,                      // ulcx_decode_crops_*: c.B rows that each name a file of `corpus`, found by the indexed walk (k_dscan_rows)
    ULCX_DEC_SAMPLES,                    // ulcx_decode_crops_samples_*: crops whose rows come from `samp`; the synthesis stores by sample (SynSamples)
    ULCX_DEC_LOWRATE,                    // ulcx_decode_crops_lowrate_*: that, with the rows and the synthesis at the geometry of `low` (SynLow)
    ULCX_DEC_PART,                       // ulcx_decode_crops_part_*: that (lgD 0 included), over every other coded channel and without the un-mix (`part`, SynPart)
    ULCX_DEC_SPECTRA,                    // ulcx_decode_crops_spectra_*: the crop walk, then k_dspec in place of the synthesis (`spec`; c.pcm / c.pcm16 both NULL)
    ULCX_DEC_DISTORTION,                 // ulcx_decode_crops_distortion_*: the crop walk, then k_ddist on the same grid (`dist`, with spec.wc / spec.lr)
    ULCX_DEC_SYNTH                       // ulcx_synth_spectra_*: no walk at all; k_synth_rows, then the synthesis from the planes of `syn` (SynPlanes); c.in is not looked at
};
static inline bool ulcx_dec_has_corpus(UlcxDecKind k) { return k >= ULCX_DEC_CROPS && k <= ULCX_DEC_DISTORTION; }
static inline bool ulcx_dec_has_synthesis(UlcxDecKind k) { return k != ULCX_DEC_SPECTRA && k != ULCX_DEC_DISTORTION; }
// What a call's launch needs beside its UlcxDecCtx: the kind, the plan of the synthesis grid, and per kind the fields named above
struct UlcxDecAux {
    UlcxDecKind kind = ULCX_DEC_PLAIN;
    int synGrid = 0;                     // > 0: workgroups of the synthesis over a cut of the (stream, block) pairs; 0: one per stream
    int synFull = 0;                     // of those, the leading ones that take one whole stream each (0: an even cut of everything)
    // kinds with a corpus (CROPS .. DISTORTION): c.rFirst and these describe the rows; c.payStride, c.payBytes and c.rIndex* are not looked at
    UlcxCorpus corpus = {};
    const int32_t *cropFile = nullptr;   // [c.B] file of each row
    const int32_t *cropCount = nullptr;  // [c.B] leading blocks wanted of each row, or NULL: all of them
    // k_crop_sample_rows first turns the caller's (start, len) rows into the decoder-owned arrays ([nStreams] each): c.rFirst is `first`
    // and cropCount is `count`, so the crop walk runs on them as on a caller's, and the synthesis clips its stores by skip / lenC /
    // nSamples.  (SYNTH: k_synth_rows writes skip / lenC; nSamples = the output blocks x BlockSize.)
    // start, len: [c.B] first sample of each row in its file's decoded stream; samples wanted of it, or NULL: nSamples, the samples per plane of the output
    struct Samp { const int64_t *start; const int32_t *len; int nSamples; int32_t *first, *count, *skip, *lenC; } samp = {};
    struct Spec { float *coef; int32_t *wc; int lr; } spec = {};   // [c.B][C][c.K - 1][BS] dequantised coefficients, channels-first; [c.B][c.K - 1] window codes (0: not live); pairs as m + s, m - s
    struct Dist {                        // the sums of the coefficients against the caller's reference planes instead of the coefficients
        double *out;                     // [c.B][C][c.K - 1][seg][3] {S, Y, E}
        const float *ref;                // [nRef][C][refBlocks][BS] reference planes, or NULL: none
        int nRef, refBlocks, seg; const int32_t *refRow, *refFirst;     // [c.B] optional, untrusted: the reference row / first reference block of each row
    } dist = {};
    struct Syn {                         // k_synth_rows turns the window codes into the per-block rows a range synthesis reads
        const float *coef; const int32_t *wc;           // [c.B][C][planes][BS] the caller's planes; [c.B][planes] their window codes (untrusted)
        int planes, lr;                  // planes per row: c.K with the plane in front (ULCX_SYNTH_WARM), else c.K - 1; lr: they hold left/right, no un-mix
    } syn = {};
    // what of the context of BlockSize >> lgD differs from the object's (the rest of it - the per-block rows, the records, their
    // strides - stays the walk's); synGrid / synFull are planned for THAT kernel
    struct Low { int lgD; UlcxTables T; int fast, twInLds; float *lapScratch; } low = {};      // lapScratch [cut workgroups][C][(BS >> lgD) / 2]
    struct Part { int which, planes; } part = {};   // PART (beside `low`: the geometry, and whether it takes the one-wave kernel): ULCX_PART_MID / _SIDE; planes of an output row, ulcx_part_channels
};
int ulcx_dec_launch(const UlcxDecCtx &c, hipStream_t st, hipEvent_t *ev, const UlcxDecAux &aux);
// block index of packed payloads (c.in / payStride / payBytes / inBytes set as for a packed call; no stream state is touched)
int ulcx_index_launch(const UlcxDecCtx &c, int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, hipStream_t st);
// the same for c.B files back to back in c.in (c.inBytes: all of it), found through offset tables of c.B + 1 entries
int ulcx_index_ragged_launch(const UlcxDecCtx &c, const int64_t *d_payOffs, const int64_t *d_idxOffs, long long idxTotal, ulcx_index_entry *d_index,
                             int32_t *d_nBlocks, hipStream_t st);
// block index of slot-form buffers: open nRows rows; append nBlocks blocks per row (c.in / c.slot / c.inBytes set as for a
// slot-form call of nRows streams; geometry and tables are all else that is read of c)
int ulcx_index_begin_launch(int nRows, ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, hipStream_t st);
int ulcx_index_slots_launch(const UlcxDecCtx &c, int nRows, int nBlocks, const int32_t *d_bits, ulcx_index_entry *d_index, int indexStride,
                            int32_t *d_nBlocks, hipStream_t st);
// corpus splice (ulcx_corpus_splice_*): the source corpus, the segment list and the outputs; five launches, no scratch
struct UlcxSpliceArgs {
    UlcxCorpus src;
    int nOut, nSeg; const int32_t *segOffs; const ulcx_segment *seg; int32_t *segStart;
    uint8_t *outPay; long long outPayStride; int32_t *outPayBytes, *outMaxBlock;
    ulcx_index_entry *outIndex; int outIndexStride; int32_t *outIndexBlocks;
};
int ulcx_splice_launch(const UlcxDecCtx &c, const UlcxSpliceArgs &a, hipStream_t st);
size_t ulcx_dec_lds_bytes(int BS, int fast, int twInLds, int listBS = 0, int oneWave = 0);   // listBS: the BlockSize the per-wave lists are sized by (0: BS); oneWave: k_dpart's carve
size_t ulcx_spec_lds_bytes(int BS);               // k_dspec's / k_ddist's dynamic LDS: two unit arrays where a CU holds them, else one
int ulcx_spec_arrays(int BS);                     // how many that is (1: ULCX_SPECTRA_LR cannot be formed on chip by k_ddist)
enum UlcxSynKind { ULCX_SYN_WHOLE, ULCX_SYN_CUT, ULCX_SYN_RANGE, ULCX_SYN_SAMPLES, ULCX_SYN_PLANES, ULCX_SYN_PLANES_LR, ULCX_SYN_LOW, ULCX_SYN_PART };   // the synthesis modes (ulcx_dec.hip: SynWhole .. SynPart)
int ulcx_dec_syn_slots(const UlcxDecCtx &c, UlcxSynKind kind, int walkBS = 0);   // resident workgroups of that mode's stereo synthesis kernel on the current device (ULCX_SYN_LOW: walkBS, the walk's BlockSize)
int ulcx_pack_launch(int nStreams, int nBlocks, int slotBytes, const uint8_t *d_slots, const int32_t *d_bits, uint8_t *d_payload,
                     long long stride, int32_t *d_payloadBytes, int32_t *d_maxBlock, hipStream_t st);
// clips (ulcx_clips.hip): the kernels around the launch sequence of ulcx_encode_clips_* - the shadow state of n rows to the state
// right after create and the caller's byte counts to 0; planar samples of blocks [k0, k0 + K) of every row into the interleaved
// staging chunk (exactly one of d_pcm / d_pcm16); the chunk's sizes masked and its kept slots appended to the payloads
// nOut: the byte counters to zero (the call's files, rows x rungs); sum: the rows' complexity sums of an analysis pass to zero, or NULL
int ulcx_clips_begin_launch(float *hist, UlcxWcState *wcs, int n, int C, int BS, int nOut, int32_t *d_payloadBytes, int32_t *d_maxBlock, double *sum, hipStream_t st);
int ulcx_clips_stage_launch(const float *d_pcm, const int16_t *d_pcm16, const int32_t *d_len, int nSamples, int n, int C, int BS, int k0, int K,
                            float *stage, hipStream_t st);
// file r * n + i: row i under rung r; slots / bits / the caller's arrays are [nRungs * n]...
int ulcx_clips_append_launch(int n, int nRungs, int K, int k0, int BS, int nSamples, const int32_t *d_len, int slot, const uint8_t *slots, int32_t *bits,
                             uint8_t *d_payload, long long stride, int32_t *d_payloadBytes, int32_t *d_maxBlock, int indexStride, const int32_t *d_indexBlocks,
                             hipStream_t st);
// the analysis pass of a clips ladder call with ULCX_RUNG_AUTO rungs: a chunk's complexities into the rows' ordered binary64 sums;
// behind the last chunk the averages (d_avg optional) and the AUTO rungs' tables, tables [ULCX_MAX_RUNGS][n]
int ulcx_clips_cplx_sum_launch(int n, int K, int k0, int BS, int nSamples, const int32_t *d_len, const float *cplx, double *sum, hipStream_t st);
int ulcx_clips_auto_launch(int n, int BS, int nSamples, const int32_t *d_len, const double *sum, const ulcx_rung *rungs, int nRungs, ulcx_rate *tables, float *d_avg,
                           hipStream_t st);
// the tap of ulcx_analyse_clips_* / ulcx_encode_clips_spectra_*: blocks [k0, k0 + kOut) of every row's planes (k0 + kOut <= nBlocks)
// from the chunk's coef [n][K][C][BS], wc [n][K] and cplx [n][K]; a block at or behind K, or behind the row's own count, is zeros
int ulcx_clips_spec_launch(int n, int K, int k0, int kOut, int C, int BS, int nSamples, const int32_t *d_len, const float *coef, const int32_t *wc,
                           const float *cplx, int nBlocks, int lr, float *d_coef, int32_t *d_wc, float *d_cplx, hipStream_t st);
// strided corpus -> ragged corpus (ulcx_clips.hip): the offsets, then a file per workgroup
int ulcx_corpus_ragged_launch(int nFiles, const uint8_t *d_payload, long long stride, const int32_t *d_payloadBytes, const ulcx_index_entry *d_index,
                              int indexStride, const int32_t *d_indexBlocks, uint8_t *d_outPayload, long long payloadCap, int64_t *d_payloadOffs,
                              ulcx_index_entry *d_outIndex, long long indexCap, int64_t *d_indexOffs, int32_t *d_outIndexBlocks, int64_t *d_need, hipStream_t st);
int ulcx_analyse_launch(const UlcxEncCtx &c, hipStream_t st, hipEvent_t *ev, const UlcxEncAux &aux, int useKxf);   // ulcx_analyse_dev; useKxf: the encode call's transform instead of the MDCT-only one (timing comparisons)
int ulcx_enc_nsums_slots(int BS, int C);                 // resident workgroups of k_nsums on the current device
// FFT array padding of k_xf (ulcx_fft.h).  One complex per 8 makes every pass conflict-free but costs 2 KB of LDS at
// BlockSize 2048 and with it the 4th workgroup per CU: measured 2.13 ms vs 1.88 ms with one per 16.
__host__ __device__ static inline int ulcx_xf_pad_shift(int BS, int C) { (void)BS; (void)C; return 4; }
// k_select_wave: candidate keys a lane keeps once the search window is small, and the LDS words of one wave's region
// (masking levels + Bark levels first, the lanes' candidate lists later)
#define ULCX_SEL_CAP 8
#ifndef ULCX_SEL_CAND
#define ULCX_SEL_CAND 128
#endif
__host__ __device__ static inline int ulcx_sel_lds_words(int BS) { int a = BS / 2 + 4 * ULCX_NBARK, b = ULCX_SEL_CAP * 64; return a > b ? a : b; }
// Stream slots (ulcx_slots.hip): one side of a copy of single streams' state - an object's own arrays, the compact shadow
// state of a subset call, or the caller's records.  Row r of the large array is at big + r * bigStride, word w of small array
// a at small[a] + r * smallStride + 4 * w (encoder: one array, the UlcxWcState; decoder: lastSub, seed, dead, packOff).
struct UlcxSlotRows {
    uint8_t *hdr; size_t hdrStride;      // records only: the 16-byte header (NULL: none)
    uint8_t *big; size_t bigStride;      // hist / lap: 16-byte aligned rows
    uint8_t *small[4]; size_t smallStride;
};
struct UlcxSlotGeom {
    int B;                               // slots of the object: list entries outside [0, B) are not the object's
    int rowVec;                          // 16-byte vectors of a large row
    int isEnc, nSmall, smallWords;       // small arrays and the words of each
    int padWords;                        // gather: words written per small array (>= smallWords; zeros behind the state)
    uint4 header;                        // gather into records: written; scatter from records: a row whose header differs is skipped
};
int ulcx_slots_gather(const UlcxSlotRows &obj, const UlcxSlotRows &rows, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st);
int ulcx_slots_scatter(const UlcxSlotRows &obj, const UlcxSlotRows &rows, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st);
int ulcx_slots_reset(const UlcxSlotRows &obj, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st);
void ulcx_enc_finalize_keys(const UlcxEncCtx &c, hipStream_t st);
void ulcx_enc_materialise_noise(const UlcxEncCtx &c, hipStream_t st);     // parity tap: the {w, w*log} pairs of the last call into c.npair
