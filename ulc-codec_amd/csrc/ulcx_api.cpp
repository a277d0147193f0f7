// ulcx_api.cpp — C ABI of the batched layer (include/ulc_amd.h §2): object lifetime,
// HBM layout, host-side constants, launches.  Host code only; every kernel lives in
// ulcx_enc.hip / ulcx_dec.hip.  There is no CPU fallback: if HIP cannot give us a
// device, every entry point returns ULCX_ERR_NO_DEVICE.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "ulcx_internal.h"
#include "../../include/ulc_amd_lowrate.h"
#include "../../include/ulc_amd_part.h"
#include "ulcx_enc_dev.h"                 // (WaveCaps, WAVE_S*, wavecaps_lds: ulcx_encoder_debug_writer_plan)
#include "ulcx_rng_tables.h"


#define CKR(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ulcx_set_error("%s: %s", #x, hipGetErrorString(e_)); return ULCX_ERR_HIP; } } while (0)
// A refused call: ULCX_ERR_ARG, and ulcx_last_error() reads "<the entry that was called>: <why>".  Every refusal in this file
// goes through here or through one of the *_bad checkers below, which take the same `who`.
static int refuse(const char *who, const char *fmt, ...) {
    char why[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why, sizeof(why), fmt, ap);
    va_end(ap);
    ulcx_set_error("%s: %s", who, why);
    return ULCX_ERR_ARG;
}

// The single-block calls (ulcx_encode_block1 / ulcx_decode_block1): own stream, and the call's enqueue sequence captured once
// into a graph that every later call replays.  noGraph: direct launches from here on.
struct Block1Graph {
    hipStream_t stream = nullptr; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    bool graphed = false, noGraph = false;
};
static void block1_drop(Block1Graph &g) { if (g.graphed) { hipGraphExecDestroy(g.exec); hipGraphDestroy(g.graph); g.graphed = false; } }
// capture + instantiate on the first call (a failure of either: direct launches from then on), then replay or enqueue, and wait
template <class F> static int block1_run(Block1Graph &g, F enqueue) {
    if (!g.graphed && !g.noGraph) {
        bool ok = hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const int rc = enqueue();
            hipGraph_t gr = nullptr;
            const hipError_t ee = hipStreamEndCapture(g.stream, &gr);
            ok = (rc == ULCX_OK) && ee == hipSuccess && gr != nullptr;
            if (ok) ok = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0) == hipSuccess;
            if (ok) { g.graph = gr; g.graphed = true; }
            else if (gr) hipGraphDestroy(gr);
        }
        if (!ok) { (void)hipGetLastError(); g.noGraph = true; }
    }
    if (g.graphed) CKR(hipGraphLaunch(g.exec, g.stream));
    else { int rc = enqueue(); if (rc) return rc; }
    CKR(hipStreamSynchronize(g.stream));
    return ULCX_OK;
}

struct ulcx_encoder {
    int device = 0, B = 0, C = 0, BS = 0, rate = 0, maxK = 0;
    UlcxEncCtx ctx = {};
    void *tables = nullptr;
    std::vector<void *> allocs;
    hipEvent_t ev[ULCX_ENC_STAGES + 1] = {};
    bool evOk = false, evRecorded = false, timing = true;
    int lastK = 0;
    UlcxEncSync sync = {};    // side streams and their events (ULCX_ASYNC_FB=0: none)
    int wcPipe = 1, nXf = 0;  // window-control / transform pipeline (ULCX_WC_PIPE chunks, default 4); transform launches of the last call
    bool keysFinal = false;
    int wcSteps = -1, wcFuse = 1;     // environment switches, read once at create
    int nsSlots = 0;                  // resident workgroups of k_nsums (its persistent grid)
    int barkMost = 0;                 // most Bark bands the full-size band tables have open at one line: what sized ctx.barkRing
    bool lastAnalyse = false;         // the last call was an analysis call: no intermediates, no exact-path count to report
    int analyseKxf = 0;               // ULCX_ANALYSE_KXF=1: analysis calls run the encode call's transform (timing comparisons)
    // staging for the host-pointer API
    float *d_pcm = nullptr; uint8_t *d_out = nullptr; int32_t *d_bits = nullptr, *d_wc = nullptr; float *d_cplx = nullptr;
    ulcx_rate *d_rate = nullptr;      // [B] the per-stream table of ulcx_encode_host_rates
    int lastRungs = 0;                // rungs of the last encode call (0: none yet, or an analysis call)
    // staging of ulcx_encode_host_ladder: [ladRungs][B][maxK] slots and sizes (grown to the largest ladder seen), tables [ULCX_MAX_RUNGS][B]
    uint8_t *ladOut = nullptr; int32_t *ladBits = nullptr; ulcx_rate *ladRate = nullptr; int ladRungs = 0;
    // single-block path (ulcx_encode_block1): pinned staging, the captured launch sequence and the parameters it was captured with
    struct Block1Meta { int32_t bits, wc; float cplx; int32_t pad; UlcxWcState wcs; };
    Block1Graph b1; bool b1Init = false;
    int b1Mode = 0; float b1P0 = 0.0f, b1P1 = 0.0f; int b1Rekeys = 0;
    float *pinIn = nullptr; uint8_t *pinOut = nullptr; Block1Meta *pinMeta = nullptr;
    // stream slots: the compact shadow state of the subset calls ([B], allocated on the first one) and the device copy of a host form's list
    float *subHist = nullptr; UlcxWcState *subWcs = nullptr; int32_t *subSlots = nullptr;
    // clips (ulcx_encode_clips_*): one chunk of the call - [B][maxK] interleaved blocks, slots and sizes (allocated on the first clips call)
    // (slots and sizes: [clipRungs][B][maxK], grown to the largest clips ladder seen; the plain clips calls are one rung)
    float *clipPcm = nullptr; uint8_t *clipOut = nullptr; int32_t *clipBits = nullptr; int clipRungs = 0;
    // ULCX_RUNG_AUTO rungs of a clips ladder call: the rows' complexity sums [B] and the resolved tables [ULCX_MAX_RUNGS][B] (allocated on the first such call)
    double *clipSum = nullptr; ulcx_rate *clipRate = nullptr;
    // clip spectra (ulcx_analyse_clips_* / ulcx_encode_clips_spectra_*): the chunk's [B][maxK] window codes and complexities (allocated on the first such call)
    int32_t *clipWc = nullptr; float *clipCplx = nullptr;
};
// What a low-rate call (ulcx_decode_crops_lowrate_*) keeps per ratio, built by the first call at that ratio (dec_low): the tables of
// BlockSize >> lgD, the synthesis kernel that geometry picks, its residency and the lapping scratch a cut of it works in.
struct UlcxDecLow {
    bool ready = false;
    void *tables = nullptr; UlcxTables T = {};
    int fastOK = 0, twInLds = 0, synSlots = 0, scratchRows = 0;
    float *lapScratch = nullptr;
};
struct ulcx_decoder {
    int device = 0, B = 0, C = 0, BS = 0, maxK = 0;
    UlcxDecCtx ctx = {};
    void *tables = nullptr;
    std::vector<void *> allocs;
    hipEvent_t ev[ULCX_DEC_STAGES + 1] = {};
    bool evOk = false, evRecorded = false, timing = true;
    uint8_t *d_in = nullptr; size_t d_in_bytes = 0; float *d_pcm = nullptr; int32_t *d_bits = nullptr;
    uint8_t *d_pay = nullptr; int32_t *d_payBytes = nullptr; long long payStride = 0;     // resident packed payloads (ulcx_decoder_upload_payload)
    // block index of the resident payloads (ulcx_decoder_index_resident) and the staged range starts of the host-pointer range entries
    ulcx_index_entry *d_index = nullptr; int32_t *d_idxBlocks = nullptr, *d_first = nullptr; int idxStride = 0;
    int32_t *bitsScr = nullptr;                                   // [B][maxK] block sizes of a range call's rows (the scan's; the caller's array has no row for the block in front)
    // k_dsyn over an even cut of the call's (stream, block) pairs: the second set of state arrays, the resident
    // workgroups of the kernel on this device, ULCX_DSYN_SPLIT=0 switches it off
    float *lap2 = nullptr; int *lastSub2 = nullptr; uint32_t *seed2 = nullptr; int *dead2 = nullptr;
    int synSlots = 0, scratchRows = 0, lastGrid = 0, lastFull = 0; bool splitOK = false, tailCut = true, rangeEvenFirst = false;
    // single-block path (ulcx_decode_block1)
    Block1Graph b1; bool b1Init = false; int b1Slot = 0;
    uint8_t *pinIn = nullptr; float *pinPcm = nullptr; int32_t *pinMeta = nullptr;
    uint32_t b1Seed = 0;                                          // the stream's RNG state between single-block calls
    // The device word (ctx.seed) is the authoritative state of the object's own noise chain; b1Seed is its host copy, which the
    // single-block path uploads in front of every block.  Any OTHER decode call on this object advances the device word only:
    // it marks the copy stale, and the next single-block call without a caller-owned state reads the device word back first.
    bool b1SeedStale = false, inBlock1 = false;
    // stream slots: the compact shadow state of the subset calls ([B], allocated on the first one; set 1 is where a cut
    // synthesis leaves its result, as lap2 .. dead2 are for the object's own arrays) and the device copy of a host form's list
    float *subLap[2] = {}; int *subLastSub[2] = {}; uint32_t *subSeed[2] = {}; int *subDead[2] = {}; int *subPackOff = nullptr;
    int32_t *subSlots = nullptr;
    UlcxDecLow low[4];                                            // [lgD] (entry 0 is never used: lgD 0 is the sample-crop call)
    int32_t *sampRows = nullptr;                                  // [4][B] a sample-crop call's rows as k_crop_sample_rows leaves them: first, count, skip, len (allocated with the shadow state)
};

#ifndef ULCX_SRC_REV
#define ULCX_SRC_REV "unknown"
#endif
extern "C" const char *ulcx_build_rev(void) { return ULCX_SRC_REV; }
extern "C" int ulcx_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { ulcx_set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return 0; }
    return n;
}

static int validate(int C, int BS) {                 // ulcEncoder.c:32-34 / ulcDecoder.c:33-35
    if (C < 1 || C > 255) return 0;
    if (BS < 256 || BS > 32768) return 0;
    if ((BS & (-BS)) != BS) return 0;
    return 1;
}
static int ilog2i(int x) { int r = 0; while ((1 << r) < x) r++; return r; }

// Alignment of the caller's device pointers (include/ulc_amd.h, "Caller buffers"): each value is the widest access a kernel
// makes to that buffer - 16 bytes for binary32 samples (float4 loads of the transform's fold, float4 stores of the
// synthesis), 8 for PCM16 samples (short4), for rate tables (float2) and for int64 offset tables, 4 for the int32 / binary32 / index arrays; the
// byte streams (slots, payloads) need none.  A NULL (optional) pointer passes.  Checked by every _dev entry before any device
// work, so that a refused call leaves the object's state as it was.
enum { ULCX_ALIGN_PCM = 16, ULCX_ALIGN_PCM16 = 8, ULCX_ALIGN_RATE = 8, ULCX_ALIGN_OFFS = 8, ULCX_ALIGN_WORD = 4 };
static bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static int misaligned(const char *who, const char *what, const void *p, int a) {
    if (aligned_to(p, (uintptr_t)a)) return 0;
    ulcx_set_error("%s: %s (%p) is not aligned to %d bytes", who, what, p, a);
    return 1;
}

template <typename T>
static int dalloc(std::vector<void *> &v, T **p, size_t count, bool zero) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { ulcx_set_error("hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); return ULCX_ERR_NOMEM; }
    if (zero) { e = hipMemset(q, 0, bytes); if (e != hipSuccess) { ulcx_set_error("hipMemset: %s", hipGetErrorString(e)); hipFree(q); return ULCX_ERR_HIP; } }
    v.push_back(q);
    *p = (T *)q;
    return ULCX_OK;
}
#define DA(ptr, count, zero) do { int rc_ = dalloc(e->allocs, &(ptr), (size_t)(count), zero); if (rc_) { cleanup(e); return rc_; } } while (0)
// Ownership: every device pointer an object owns is in its `allocs`, which cleanup() frees in one loop.  A buffer that
// grows or is replaced during the object's life goes through dregrow: the old one is freed and leaves the list first, and a
// failed allocation leaves *p == nullptr.  Buffers that live for one call are a DevTmp's.
template <typename T>
static void dfree(std::vector<void *> &v, T **p) {
    if (!*p) return;
    v.erase(std::remove(v.begin(), v.end(), (void *)*p), v.end());
    hipFree((void *)*p);
    *p = nullptr;
}
template <typename T>
static int dregrow(std::vector<void *> &v, T **p, size_t count, bool zero) { dfree(v, p); return dalloc(v, p, count, zero); }
namespace { struct DevTmp { std::vector<void *> v; ~DevTmp() { for (void *p : v) hipFree(p); } template <typename T> hipError_t get(T **p, size_t bytes) { void *q = nullptr; hipError_t r = hipMalloc(&q, bytes ? bytes : 16); if (r == hipSuccess) v.push_back(q); *p = (T *)q; return r; } }; }

static int select_device(const char *who, int device) {
    int n = ulcx_device_count();
    if (n <= 0) { if (!ulcx_last_error()[0]) ulcx_set_error("no HIP device visible"); return ULCX_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) return refuse(who, "device %d out of range (have %d)", device, n);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { ulcx_set_error("hipSetDevice: %s", hipGetErrorString(e)); return ULCX_ERR_NO_DEVICE; }
    return ULCX_OK;
}

// ---------------------------------------------------------------------------
// encoder
// ---------------------------------------------------------------------------
// The side streams and every event of UlcxEncSync: all of them or none.  Only the transform's timing pairs can be timed.
static const size_t kEncSyncUntimed = offsetof(UlcxEncSync, xfTiming) / sizeof(hipEvent_t);
static void enc_sync_destroy(UlcxEncSync &s) {
    hipEvent_t *ev = &s.wcStart;
    for (size_t i = 0; i < kEncSyncUntimed + 2 * ULCX_XF_MAXCH; i++) if (ev[i]) hipEventDestroy(ev[i]);
    for (hipStream_t st : { s.side, s.side2, s.side3 }) if (st) hipStreamDestroy(st);
    s = UlcxEncSync{};
}
static bool enc_sync_create(UlcxEncSync &s) {
    static_assert(offsetof(UlcxEncSync, wcStart) == 0 && offsetof(UlcxEncSync, side) == (kEncSyncUntimed + 2 * ULCX_XF_MAXCH) * sizeof(hipEvent_t), "UlcxEncSync: events, then streams");
    hipEvent_t *ev = &s.wcStart;
    bool ok = true;
    for (hipStream_t *st : { &s.side, &s.side2, &s.side3 }) ok = ok && hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess;
    for (size_t i = 0; i < kEncSyncUntimed; i++) ok = ok && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    for (auto &v : s.xfTiming) ok = ok && hipEventCreate(&v) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); enc_sync_destroy(s); }
    return ok;
}

static void cleanup(ulcx_encoder *e) {
    if (!e) return;
    for (void *p : e->allocs) hipFree(p);
    if (e->tables) hipFree(e->tables);
    if (e->evOk) for (auto &v : e->ev) hipEventDestroy(v);
    block1_drop(e->b1);
    if (e->b1.stream) hipStreamDestroy(e->b1.stream);
    if (e->pinIn) hipHostFree(e->pinIn);
    if (e->pinOut) hipHostFree(e->pinOut);
    if (e->pinMeta) hipHostFree(e->pinMeta);
    enc_sync_destroy(e->sync);
    delete e;
}

static int enc_reset_state(ulcx_encoder *e) {
    UlcxEncCtx &c = e->ctx;
    CKR(hipMemset(c.hist, 0, sizeof(float) * (size_t)e->B * 2 * e->BS * e->C));
    std::vector<UlcxWcState> w((size_t)e->B);
    for (auto &x : w) {
        memset(&x, 0, sizeof(x));
        x.wcPrev = 0x10;              // virtual block -1: full-size, full-overlap
        x.wcCur  = 0x10;              // State->NextWindowCtrl = 0x10 (ulcEncoder.c:70)
    }
    CKR(hipMemcpy(c.wcs, w.data(), sizeof(UlcxWcState) * w.size(), hipMemcpyHostToDevice));
    return ULCX_OK;
}

extern "C" int ulcx_encoder_create(ulcx_encoder **out, int device, int nStreams, int nChan, int BlockSize, int RateHz, int maxBlocksPerCall) {
    const char *who = "ulcx_encoder_create";
    if (!out) return refuse(who, "no place for the object");
    *out = nullptr;
    if (!validate(nChan, BlockSize) || nStreams < 1 || maxBlocksPerCall < 1 || RateHz < 1)
        return refuse(who, "invalid encoder geometry (nStreams=%d nChan=%d BlockSize=%d RateHz=%d maxBlocks=%d)", nStreams, nChan, BlockSize, RateHz, maxBlocksPerCall);
    if (BlockSize > ULCX_MAX_BS_DEVICE) { ulcx_set_error("BlockSize %d > %d not built for the device yet", BlockSize, ULCX_MAX_BS_DEVICE); return ULCX_ERR_UNSUPPORTED; }
    int rc = select_device(who, device);
    if (rc) return rc;
    ulcx_encoder *e = new ulcx_encoder();
    e->device = device; e->B = nStreams; e->C = nChan; e->BS = BlockSize; e->rate = RateHz; e->maxK = maxBlocksPerCall;
    UlcxEncCtx &c = e->ctx;
    c.B = nStreams; c.C = nChan; c.BS = BlockSize; c.lgBS = ilog2i(BlockSize); c.maxK = maxBlocksPerCall; c.K = 0;
    c.rateHz = RateHz;
    c.slot = 2 * nChan * BlockSize + 16;          // >= worst case 4 nybbles/coefficient + header
    c.unitCap = 2 * BlockSize + 32;
    // data-independent libm calls of the reference, evaluated on the host like the reference does
    c.cHP  = 1.0f - expf(-0x1.CC845Cp6f / RateHz);            // WindowControl.c:75,82
    c.cBP  = 1.0f - expf(-0x1.596344p8f / RateHz);            // :76,83
    c.qHP  = 1.0f - expf(-0x1.CC845Cp7f / RateHz);            // :94,101
    c.qBP  = 1.0f - expf(-0x1.596344p8f / RateHz);            // :95,102
    c.cBlk = 1.0f - expf(-0x1.1AF110p-6f * BlockSize / RateHz); // :120,126
    c.cplxScale = 0x1.62E430p-1f * (31 - __builtin_clz((unsigned)BlockSize));   // BlockTransform.c:320
    rc = ulcx_tables_build(&c.T, &e->tables, BlockSize, RateHz, true);
    if (rc) { cleanup(e); return rc; }
    c.barkRing = ulcx_tables_bark_ring(c.T, BlockSize, &e->barkMost);
    // (round 3: the ring kernels also for a few blocks per call - the drop-in's one: the four-wave kernel walks a row's 1024 lines in
    //  a quarter of the time the lane-per-subblock kernels take, which is what a single stream waits for)
    size_t B = nStreams, K = maxBlocksPerCall, NB = B * K, cb = (size_t)nChan * BlockSize;
    DA(c.hist, B * 2 * BlockSize * nChan, true);
    DA(c.wcs, B, true);
    DA(c.env, ((B + 63) / 64) * 64 * K * BlockSize, true);
    DA(c.bins, B * (K + 1) * 16, true);
    DA(c.wcArr, B * (K + 2), true);
    DA(c.coef, NB * cb, false);
    DA(c.key, NB * cb, false);
    DA(c.nsum, ((NB * nChan + 63) / 64) * 64 * (size_t)(BlockSize / 2), false);      // rows in tiles of 64 (tile_idx)
    DA(c.amp2, ((NB + 63) / 64) * 64 * (size_t)(BlockSize / 2), false);
    DA(c.barkN, NB * nChan * 4 * ULCX_NBARK, true);
    DA(c.barkP, NB * 4 * ULCX_NBARK, true);
    if (c.barkRing) { DA(c.barkRawN, NB * nChan * ULCX_NBARK * 3, false); DA(c.barkRawP, NB * ULCX_NBARK * 3, false); DA(c.decList, NB, false); DA(c.decCount, 1, true); }
    DA(c.nnz, NB, true);
    DA(c.cplx, NB, true);
    DA(c.nout, NB, true);
    DA(c.slow, 3 * NB + 2, true);                      // flags [NB], retry-queue counters [2], retry queues [2][NB]
    c.useWave = 1;        // wave-per-unit encode pass fed by k_nsums / k_tails; the serial lane-per-unit kernel takes what its capacities cannot hold
    c.useGapSums = (cb <= 16384 && nChan <= 16) ? 1 : 0;          // (k_nsums: a block's pairs in LDS, two bits per channel in a word)
    DA(c.gapSum, NB * cb, false);
    DA(c.tailSum, NB * nChan * 4 * 8, true);
    c.directPack = 1;
    if (const char *ev = getenv("ULCX_DIRECT_PACK")) c.directPack = (ev[0] != '0');
    c.dbgSkip = 0;
#ifdef ULCX_ABLATE
    if (const char *ev = getenv("ULCX_DBG_SKIP")) c.dbgSkip = atoi(ev);   // timing experiments only (breaks results)
#endif
    DA(c.cbrLo, NB, true); DA(c.cbrHi, NB, true); DA(c.cbrDone, NB, true); DA(c.cbrBudget, NB, true); DA(c.cbrLive, 1, true);
    DA(c.selWin, NB, true); DA(c.selT, NB, true); c.selPass = 0;
    { const char *ev = getenv("ULCX_SEL_PAIR"); c.selPair = ev ? atoi(ev) : 1; }
    DA(c.keep, NB * cb / 32, true);
    DA(c.fbList, NB, true);
    DA(c.fbCount, 4, true);
    DA(c.unitBuf, NB * nChan * (size_t)c.unitCap, true);
    DA(c.unitNyb, NB * nChan * 4, true);
    {
        size_t heapBytes = (cb * 8 > ULCX_HEAP_LDS_BYTES) ? (size_t)ULCX_HEAP_GRID * cb * 8 : 16;
        uint8_t *hp = nullptr;
        DA(hp, heapBytes, false);
        c.heapScratch = hp;
    }
    for (auto &v : e->ev) { if (hipEventCreate(&v) != hipSuccess) { ulcx_set_error("hipEventCreate failed"); cleanup(e); return ULCX_ERR_HIP; } }
    e->evOk = true;
    {
        const char *evs = getenv("ULCX_ASYNC_FB");
        const bool sideOk = !(evs && evs[0] == '0') && enc_sync_create(e->sync);
        e->wcPipe = sideOk ? 4 : 1;                            // transform chunks per call: 1 block, then thirds (4 vs 5 chunks: 9.50 vs 9.56 ms per bench step)
        if (const char *pv = getenv("ULCX_WC_PIPE")) { int n = atoi(pv); if (n >= 1 && n <= ULCX_XF_MAXCH && n != 2 && (n == 1 || sideOk)) e->wcPipe = n; }
        if (const char *sv = getenv("ULCX_WC_STEPS")) e->wcSteps = atoi(sv);      // -1: default; 0: the transform's chunks
        // (wcFuse = 1: stereo k_wc_ef; every other channel count: k_wc_energy + k_wc_forward)
    }
    if (const char *av = getenv("ULCX_ANALYSE_KXF")) e->analyseKxf = (av[0] == '1');
    e->nsSlots = c.useGapSums ? ulcx_enc_nsums_slots(BlockSize, nChan) : 0;
    if (e->nsSlots <= 0) e->nsSlots = 1024;
    DA(c.isFb, NB, true);
    DA(c.ownSlot, NB, true);
    {
        // Rank slots of the exact path (one full ranking per tie-straddle block).  One slot per block while that stays
        // within 8 GiB (a rate-search call over 524 288 blocks with 1 GiB of slots enqueued the exact path's fifteen passes
        // for eight groups of slots, seven of them always empty) AND within a quarter of what the device has free right
        // now: several encoders may share one GPU (`ulcx-tool -devices:N` above the visible count, two host threads, eight
        // test ranks).  ULCX_RANK_SLOTS=n overrides (tests).  If the allocation fails all the same, halve down to 64 slots
        // rather than fail the create: the launch walks groups of slots whatever their number (ulcx_enc_launch).
        size_t slots = NB;
        size_t maxSlots = ((size_t)8 << 30) / (cb * 4);
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB / 4 / (cb * 4) < maxSlots) maxSlots = freeB / 4 / (cb * 4);
        if (maxSlots < 64) maxSlots = 64;
        if (slots > maxSlots) slots = maxSlots;
        if (const char *ev = getenv("ULCX_RANK_SLOTS")) { long n = atol(ev); if (n >= 1 && (size_t)n < slots) slots = (size_t)n; }
        for (;;) {
            int rc_ = dalloc(e->allocs, &c.rankBuf, slots * cb, false);
            if (rc_ == ULCX_OK) break;
            if (rc_ != ULCX_ERR_NOMEM || slots <= 64) { cleanup(e); return rc_; }
            (void)hipGetLastError();
            slots = (slots + 1) / 2; if (slots < 64) slots = 64;
        }
        c.rankSlots = (int)slots;
    }
    rc = enc_reset_state(e);
    if (rc) { cleanup(e); return rc; }
    *out = e;
    return ULCX_OK;
}

extern "C" void ulcx_encoder_destroy(ulcx_encoder *e) { if (e) { hipSetDevice(e->device); cleanup(e); } }
extern "C" int ulcx_encoder_reset(ulcx_encoder *e) { if (!e) return refuse("ulcx_encoder_reset", "no encoder"); CKR(hipSetDevice(e->device)); return enc_reset_state(e); }
extern "C" int ulcx_encoder_slot_bytes(const ulcx_encoder *e) { return e ? e->ctx.slot : 0; }

// What a call of nBlocks launches with.  Short calls pipeline window control and transform in fewer chunks or not at all
// (wcPipe > 1 only ever with side streams: ulcx_encoder_create).
static UlcxEncAux enc_aux(ulcx_encoder *e, int nBlocks) {
    const int wcPipe = (nBlocks >= 2 * e->wcPipe) ? e->wcPipe : (nBlocks >= 6 && e->wcPipe > 1 ? 3 : 1);
    return UlcxEncAux{ e->sync, wcPipe, e->wcSteps, e->wcFuse, e->nsSlots, e->nXf };
}

// ---- stream slots (include/ulc_amd.h): what the copies of ulcx_slots.hip work on
// a list of the device forms: checked as far as the host can see it
static int slots_list_bad(const char *who, const int32_t *d_slots, int n, int B) {
    if (!d_slots || n < 1 || n > B) { ulcx_set_error("%s: no slot list, or n = %d not in 1 .. nStreams = %d", who, n, B); return 1; }
    return misaligned(who, "d_slots", d_slots, ULCX_ALIGN_WORD);
}
// a list of the host forms: every entry a slot of the object, none twice
static int slots_host_bad(const char *who, const int32_t *h_slots, int n, int B) {
    if (!h_slots || n < 1 || n > B) { ulcx_set_error("%s: no slot list, or n = %d not in 1 .. nStreams = %d", who, n, B); return 1; }
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n; i++) {
        const int s = h_slots[i];
        if (s < 0 || s >= B) { ulcx_set_error("%s: entry %d is slot %d, outside 0 .. %d", who, i, s, B - 1); return 1; }
        if (seen[(size_t)s]) { ulcx_set_error("%s: slot %d is listed twice", who, s); return 1; }
        seen[(size_t)s] = 1;
    }
    return 0;
}
static int record_headers_bad(const char *who, const uint8_t *h_state, int n, size_t bytes, const uint4 &want) {
    for (int i = 0; i < n; i++) {
        uint32_t h[4];
        memcpy(h, h_state + (size_t)i * bytes, sizeof(h));
        if (h[0] != want.x || h[1] != want.y || h[2] != want.z || h[3] != want.w) {
            ulcx_set_error("%s: record %d is {magic %08x, nChan %u, BlockSize %u, RateHz %u}, this object takes {%08x, %u, %u, %u}", who, i,
                           h[0], h[1], h[2], h[3], want.x, want.y, want.z, want.w);
            return 1;
        }
    }
    return 0;
}
// What the slot entries need of an object, one overload per object type (the decoder's: further down): its own rows, the rows
// of saved records, the geometry of either, a record's size, and what a change of the state behind the object's back touches.
enum { ULCX_ALIGN_STATE = 16, ULCX_STATE_HEADER = 16, ULCX_WCS_WORDS = sizeof(UlcxWcState) / 4, ULCX_WCS_REC_BYTES = (sizeof(UlcxWcState) + 15) / 16 * 16 };
static size_t enc_hist_bytes(const ulcx_encoder *e) { return sizeof(float) * 2 * (size_t)e->BS * e->C; }
extern "C" size_t ulcx_encoder_stream_state_bytes(const ulcx_encoder *e) { return e ? ULCX_STATE_HEADER + enc_hist_bytes(e) + ULCX_WCS_REC_BYTES : 0; }
static size_t slot_state_bytes(const ulcx_encoder *e) { return ulcx_encoder_stream_state_bytes(e); }
static void slot_touch(ulcx_encoder *) {}
static UlcxSlotGeom slot_geom(const ulcx_encoder *e, bool record) {
    UlcxSlotGeom g = {};
    g.B = e->B; g.rowVec = (int)(enc_hist_bytes(e) / 16); g.isEnc = 1; g.nSmall = 1; g.smallWords = ULCX_WCS_WORDS;
    g.padWords = record ? ULCX_WCS_REC_BYTES / 4 : ULCX_WCS_WORDS;
    g.header = make_uint4(ULCX_STATE_MAGIC_ENC, (unsigned)e->C, (unsigned)e->BS, (unsigned)e->rate);
    return g;
}
static UlcxSlotRows enc_slot_rows(const ulcx_encoder *e, float *hist, UlcxWcState *wcs) {
    UlcxSlotRows r = {};
    r.big = (uint8_t *)hist; r.bigStride = enc_hist_bytes(e); r.small[0] = (uint8_t *)wcs; r.smallStride = sizeof(UlcxWcState);
    return r;
}
static UlcxSlotRows slot_obj_rows(const ulcx_encoder *e) { return enc_slot_rows(e, e->ctx.hist, e->ctx.wcs); }
static UlcxSlotRows slot_record_rows(const ulcx_encoder *e, uint8_t *state) {
    UlcxSlotRows r = {};
    const size_t bytes = slot_state_bytes(e);
    r.hdr = state; r.hdrStride = bytes; r.big = state + ULCX_STATE_HEADER; r.bigStride = bytes;
    r.small[0] = state + ULCX_STATE_HEADER + enc_hist_bytes(e); r.smallStride = bytes;
    return r;
}
static int enc_shadow(ulcx_encoder *e) {
    int rc;
    if (!e->subHist && (rc = dalloc(e->allocs, &e->subHist, (size_t)e->B * 2 * e->BS * e->C, false))) return rc;
    if (!e->subWcs && (rc = dalloc(e->allocs, &e->subWcs, (size_t)e->B, false))) return rc;
    return ULCX_OK;
}

// ---- the encoder's call families.  A public entry is a wrapper that names itself (`who`) to the body of its family:
//   encode_dev_any     plain, _pcm16, _rates and _subset calls        encode_ladder_any   the ladder
//   analyse_dev_any    analysis calls, whole object or subset
// A body makes every check before any device work - so a refused call leaves the object as it was - and names `who` in every
// message.  The host-pointer forms make their own checks first (through the same checkers), then: staging (host_staging),
// input up (enc_pcm_up), the body on the null stream, results down (enc_results_down).
static bool mode_ok(int m) { return m == ULCX_MODE_VBR || m == ULCX_MODE_CBR || m == ULCX_MODE_ABR; }
// the arguments every entry of the encoder has: pcm = the one sample pointer the entry takes, device or host
static int enc_args_bad(const char *who, const ulcx_encoder *e, const void *pcm, bool haveOut, int nBlocks) {
    if (!e || !pcm || !haveOut) { refuse(who, "bad argument"); return 1; }
    if (nBlocks < 1 || nBlocks > e->maxK) { refuse(who, "nBlocks out of range"); return 1; }
    return 0;
}
// the one validator of a {RateKbps, AvgComplexity} pair: what ulcEncodeTool.c:43-50 accepts
static int rate_entry_bad(const char *who, const char *what, int index, float r, float a) {
    if (isfinite(r) && isfinite(a) && r != 0.0f && !(a < 0.0f)) return 0;
    refuse(who, "%s %d (RateKbps %g, AvgComplexity %g)", what, index, (double)r, (double)a);
    return 1;
}
static int rate_table_bad(const char *who, const char *what, const ulcx_rate *h_rate, int n) {
    for (int i = 0; i < n; i++) if (rate_entry_bad(who, what, i, h_rate[i].RateKbps, h_rate[i].AvgComplexity)) return 1;
    return 0;
}
// The context of one call (one rung of a ladder call): the object's, with the call's setting and input.  d_rate != NULL: a
// per-stream table read on the device; the scalar setting is then VBR / 100 / 0 whatever was passed.  The outputs are the caller's.
static UlcxEncCtx enc_call_ctx(const ulcx_encoder *e, int mode, float p0, float p1, const ulcx_rate *d_rate, const float *d_pcm, const int16_t *d_pcm16, int nBlocks) {
    UlcxEncCtx c = e->ctx;
    if (d_rate) { mode = ULCX_MODE_VBR; p0 = 100.0f; p1 = 0.0f; }
    c.K = nBlocks; c.keyFinal = 0; c.mode = mode; c.p0 = p0; c.p1 = p1;
    c.vbrTarget = (mode == ULCX_MODE_VBR) ? 0x1.E4EFB7p3f * logf(100.0f / p0) : 0.0f;     // ulcEncoder.c:144 (host libm, data independent)
    c.rates = (const float2 *)d_rate;
    c.pcm = d_pcm; c.pcm16 = d_pcm16; c.out = nullptr; c.bits = nullptr; c.wcOut = nullptr; c.cplxOut = nullptr;
    return c;
}
// what the object remembers of its last call
static int enc_call_done(ulcx_encoder *e, int rc, int nBlocks, bool analyse, int rungs) {
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    e->lastK = nBlocks;
    e->keysFinal = false;
    e->lastAnalyse = analyse;
    e->lastRungs = rungs;
    return rc;
}
// d_slots != NULL: a subset call - the n listed slots' state gathered into the compact shadow arrays, the plain call's launch
// sequence on those with c.B = n (every kernel takes its strides from c.B, c.K and c.maxK; the per-call scratch is sized for
// nStreams >= n), the result scattered back; all on the caller's stream, which the launch joins its side streams into.
template <class F> static int enc_launch_on(ulcx_encoder *e, UlcxEncCtx &c, const int32_t *d_slots, int n, hipStream_t st, F launch) {
    if (!d_slots) return launch(c);
    int rc = enc_shadow(e);
    if (rc) return rc;
    const UlcxSlotRows shadow = enc_slot_rows(e, e->subHist, e->subWcs);
    if ((rc = ulcx_slots_gather(slot_obj_rows(e), shadow, d_slots, n, slot_geom(e, false), st))) return rc;
    c.B = n; c.hist = e->subHist; c.wcs = e->subWcs;
    rc = launch(c);
    if (rc == ULCX_OK) rc = ulcx_slots_scatter(slot_obj_rows(e), shadow, d_slots, n, slot_geom(e, false), st);
    return rc;
}

// needRate: the entry takes a table (the _rates calls); a subset call may have one.  subset: the entry takes a slot list.
static int encode_dev_any(const char *who, ulcx_encoder *e, int mode, float p0, float p1, const ulcx_rate *d_rate, bool needRate,
                          const float *d_pcm, const int16_t *d_pcm16, int nBlocks, uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx,
                          void *hipStream, bool subset = false, const int32_t *d_slots = nullptr, int n = 0) {
    if (enc_args_bad(who, e, d_pcm ? (const void *)d_pcm : d_pcm16, d_out && d_bits && (d_rate || !needRate), nBlocks)) return ULCX_ERR_ARG;
    if (subset && slots_list_bad(who, d_slots, n, e->B)) return ULCX_ERR_ARG;
    if (!d_rate && !mode_ok(mode)) return refuse(who, "bad mode");
    if (misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16) ||
        misaligned(who, "d_rate", d_rate, ULCX_ALIGN_RATE) || misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_wc", d_wc, ULCX_ALIGN_WORD) || misaligned(who, "d_cplx", d_cplx, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxEncCtx c = enc_call_ctx(e, mode, p0, p1, d_rate, d_pcm, d_pcm16, nBlocks);
    c.out = d_out; c.bits = d_bits; c.wcOut = d_wc; c.cplxOut = d_cplx;
    const UlcxEncAux aux = enc_aux(e, nBlocks);
    const int rc = enc_launch_on(e, c, subset ? d_slots : nullptr, n, (hipStream_t)hipStream,
                                 [&](UlcxEncCtx &cc) { return ulcx_enc_launch(cc, (hipStream_t)hipStream, e->timing ? e->ev : nullptr, aux); });
    return enc_call_done(e, rc, nBlocks, false, 1);
}
extern "C" int ulcx_encode_dev(ulcx_encoder *e, int mode, float p0, float p1, const float *d_pcm, int nBlocks,
                               uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev", e, mode, p0, p1, nullptr, false, d_pcm, nullptr, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encode_dev_pcm16(ulcx_encoder *e, int mode, float p0, float p1, const int16_t *d_pcm16, int nBlocks,
                                     uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev_pcm16", e, mode, p0, p1, nullptr, false, nullptr, d_pcm16, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encode_dev_rates(ulcx_encoder *e, const ulcx_rate *d_rate, const float *d_pcm, int nBlocks,
                                     uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev_rates", e, 0, 0.0f, 0.0f, d_rate, true, d_pcm, nullptr, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encode_dev_pcm16_rates(ulcx_encoder *e, const ulcx_rate *d_rate, const int16_t *d_pcm16, int nBlocks,
                                           uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev_pcm16_rates", e, 0, 0.0f, 0.0f, d_rate, true, nullptr, d_pcm16, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encode_dev_subset(ulcx_encoder *e, const int32_t *d_slots, int n, int mode, float p0, float p1, const ulcx_rate *d_rate, const float *d_pcm, int nBlocks,
                                      uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev_subset", e, mode, p0, p1, d_rate, false, d_pcm, nullptr, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream, true, d_slots, n);
}
extern "C" int ulcx_encode_dev_pcm16_subset(ulcx_encoder *e, const int32_t *d_slots, int n, int mode, float p0, float p1, const ulcx_rate *d_rate, const int16_t *d_pcm16, int nBlocks,
                                            uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_dev_any("ulcx_encode_dev_pcm16_subset", e, mode, p0, p1, d_rate, false, nullptr, d_pcm16, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream, true, d_slots, n);
}

// ---- ladder (include/ulc_amd.h): one context per rung from the shared one; tables are device pointers here
static int ladder_bad(const char *who, const ulcx_rung *rungs, int nRungs) {
    if (!rungs || nRungs < 1 || nRungs > ULCX_MAX_RUNGS) { refuse(who, "nRungs %d not in 1 .. %d (or no rungs)", nRungs, ULCX_MAX_RUNGS); return 1; }
    for (int r = 0; r < nRungs; r++) {
        if (rungs[r].reserved != 0) { refuse(who, "rung %d: reserved must be 0", r); return 1; }
        if (!rungs[r].rate && !mode_ok(rungs[r].mode)) { refuse(who, "rung %d: bad mode %d", r, rungs[r].mode); return 1; }
    }
    return 0;
}
static int encode_ladder_any(const char *who, ulcx_encoder *e, const ulcx_rung *rungs, int nRungs, const float *d_pcm, const int16_t *d_pcm16, int nBlocks,
                             uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    if (ladder_bad(who, rungs, nRungs) || enc_args_bad(who, e, d_pcm ? (const void *)d_pcm : d_pcm16, d_out && d_bits, nBlocks)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16) ||
        misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD) || misaligned(who, "d_wc", d_wc, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_cplx", d_cplx, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    for (int r = 0; r < nRungs; r++) if (misaligned(who, "a rung's rate table", rungs[r].rate, ULCX_ALIGN_RATE)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxEncCtx cs[ULCX_MAX_RUNGS];
    const size_t NB = (size_t)e->B * nBlocks;
    for (int r = 0; r < nRungs; r++) {
        UlcxEncCtx &c = cs[r];
        c = enc_call_ctx(e, rungs[r].mode, rungs[r].param0, rungs[r].param1, rungs[r].rate, d_pcm, d_pcm16, nBlocks);
        c.out = d_out + r * NB * (size_t)c.slot; c.bits = d_bits + r * NB;
        if (!r) { c.wcOut = d_wc; c.cplxOut = d_cplx; }
    }
    const int rc = ulcx_enc_launch_ladder(cs, nRungs, (hipStream_t)hipStream, e->timing ? e->ev : nullptr, enc_aux(e, nBlocks));
    return enc_call_done(e, rc, nBlocks, false, nRungs);
}
extern "C" int ulcx_encode_dev_ladder(ulcx_encoder *e, const ulcx_rung *rungs, int nRungs, const float *d_pcm, int nBlocks,
                                      uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_ladder_any("ulcx_encode_dev_ladder", e, rungs, nRungs, d_pcm, nullptr, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encode_dev_pcm16_ladder(ulcx_encoder *e, const ulcx_rung *rungs, int nRungs, const int16_t *d_pcm16, int nBlocks,
                                            uint8_t *d_out, int32_t *d_bits, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_ladder_any("ulcx_encode_dev_pcm16_ladder", e, rungs, nRungs, nullptr, d_pcm16, nBlocks, d_out, d_bits, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_encoder_last_rungs(ulcx_encoder *e) { return e ? e->lastRungs : refuse("ulcx_encoder_last_rungs", "no encoder"); }

// ---- analysis only (include/ulc_amd.h): window control, MDCT, block complexity, next-call state
static int analyse_dev_any(const char *who, ulcx_encoder *e, const float *d_pcm, const int16_t *d_pcm16, int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream,
                           bool subset = false, const int32_t *d_slots = nullptr, int n = 0) {
    if (enc_args_bad(who, e, d_pcm ? (const void *)d_pcm : d_pcm16, d_wc || d_cplx, nBlocks)) return ULCX_ERR_ARG;
    if (subset && slots_list_bad(who, d_slots, n, e->B)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16) ||
        misaligned(who, "d_wc", d_wc, ULCX_ALIGN_WORD) || misaligned(who, "d_cplx", d_cplx, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxEncCtx c = enc_call_ctx(e, ULCX_MODE_VBR, 100.0f, 0.0f, nullptr, d_pcm, d_pcm16, nBlocks);
    c.wcOut = d_wc; c.cplxOut = d_cplx;
    const UlcxEncAux aux = enc_aux(e, nBlocks);      // (the encode call's chunking)
    const int rc = enc_launch_on(e, c, subset ? d_slots : nullptr, n, (hipStream_t)hipStream,
                                 [&](UlcxEncCtx &cc) { return ulcx_analyse_launch(cc, (hipStream_t)hipStream, e->timing ? e->ev : nullptr, aux, e->analyseKxf); });
    return enc_call_done(e, rc, nBlocks, true, 0);
}
extern "C" int ulcx_analyse_dev(ulcx_encoder *e, const float *d_pcm, int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return analyse_dev_any("ulcx_analyse_dev", e, d_pcm, nullptr, nBlocks, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_analyse_dev_pcm16(ulcx_encoder *e, const int16_t *d_pcm16, int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return analyse_dev_any("ulcx_analyse_dev_pcm16", e, nullptr, d_pcm16, nBlocks, d_wc, d_cplx, hipStream);
}
extern "C" int ulcx_analyse_dev_subset(ulcx_encoder *e, const int32_t *d_slots, int n, const float *d_pcm, int nBlocks, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return analyse_dev_any("ulcx_analyse_dev_subset", e, d_pcm, nullptr, nBlocks, d_wc, d_cplx, hipStream, true, d_slots, n);
}

// ---- host-pointer forms.  Device staging kept by the object, sized for maxBlocksPerCall blocks of every stream: input,
// window codes, complexities; withOut: output slots and sizes too (an encoder that only ever analyses never allocates those)
static int host_staging(ulcx_encoder *e, bool withOut) {
    const size_t nBlk = (size_t)e->B * e->maxK, cb = (size_t)e->C * e->BS;
    int rc;
    if (!e->d_pcm && (rc = dalloc(e->allocs, &e->d_pcm, nBlk * cb, false))) return rc;
    if (!e->d_wc && (rc = dalloc(e->allocs, &e->d_wc, nBlk, false))) return rc;
    if (!e->d_cplx && (rc = dalloc(e->allocs, &e->d_cplx, nBlk, false))) return rc;
    if (withOut && !e->d_out && (rc = dalloc(e->allocs, &e->d_out, nBlk * e->ctx.slot, false))) return rc;
    if (withOut && !e->d_bits && (rc = dalloc(e->allocs, &e->d_bits, nBlk, false))) return rc;
    return ULCX_OK;
}
// the device copy of a host form's slot list
template <class OBJ> static int slots_list_up(OBJ *e, const int32_t *h_slots, int n) {
    if (!e->subSlots) { int rc = dalloc(e->allocs, &e->subSlots, (size_t)e->B, false); if (rc) return rc; }
    CKR(hipMemcpy(e->subSlots, h_slots, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
    return ULCX_OK;
}
static int enc_pcm_up(ulcx_encoder *e, const float *h_pcm, size_t NB) {
    CKR(hipMemcpy(e->d_pcm, h_pcm, sizeof(float) * NB * (size_t)e->C * e->BS, hipMemcpyHostToDevice));
    return ULCX_OK;
}
// Waits for the device, then copies a call's results down: nSlotsDown slots and sizes from d_out / d_bits (none: an analysis
// call; a ladder call: every rung's), NB window codes and complexities from the object's staging where the caller wants them.
static int enc_results_down(ulcx_encoder *e, const uint8_t *d_out, const int32_t *d_bits, size_t nSlotsDown, size_t NB,
                            uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx) {
    CKR(hipDeviceSynchronize());
    if (h_out) CKR(hipMemcpy(h_out, d_out, nSlotsDown * e->ctx.slot, hipMemcpyDeviceToHost));
    if (h_bits) CKR(hipMemcpy(h_bits, d_bits, sizeof(int32_t) * nSlotsDown, hipMemcpyDeviceToHost));
    if (h_wc) CKR(hipMemcpy(h_wc, e->d_wc, sizeof(int32_t) * NB, hipMemcpyDeviceToHost));
    if (h_cplx) CKR(hipMemcpy(h_cplx, e->d_cplx, sizeof(float) * NB, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
extern "C" int ulcx_analyse_host(ulcx_encoder *e, const float *h_pcm, int nBlocks, int32_t *h_wc, float *h_cplx) {
    const char *who = "ulcx_analyse_host";
    if (enc_args_bad(who, e, h_pcm, h_wc || h_cplx, nBlocks)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t NB = (size_t)e->B * nBlocks;
    int rc = host_staging(e, false);
    if (!rc) rc = enc_pcm_up(e, h_pcm, NB);
    if (!rc) rc = analyse_dev_any(who, e, e->d_pcm, nullptr, nBlocks, h_wc ? e->d_wc : nullptr, h_cplx ? e->d_cplx : nullptr, nullptr);
    return rc ? rc : enc_results_down(e, nullptr, nullptr, 0, NB, nullptr, nullptr, h_wc, h_cplx);
}
// The plain, _rates and _subset host forms behind their argument checks.  h_rate: a table of one entry per row of the call;
// h_slots: a subset call of n rows.
static int encode_host_any(const char *who, ulcx_encoder *e, int mode, float p0, float p1, const ulcx_rate *h_rate, const float *h_pcm, int nBlocks,
                           uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx, const int32_t *h_slots = nullptr, int n = 0) {
    CKR(hipSetDevice(e->device));
    const size_t rows = h_slots ? (size_t)n : (size_t)e->B, NB = rows * nBlocks;
    int rc = host_staging(e, true);
    if (!rc && h_rate && !e->d_rate) rc = dalloc(e->allocs, &e->d_rate, (size_t)e->B, false);
    if (!rc && h_slots) rc = slots_list_up(e, h_slots, n);
    if (rc) return rc;
    if (h_rate) CKR(hipMemcpy(e->d_rate, h_rate, sizeof(ulcx_rate) * rows, hipMemcpyHostToDevice));
    if ((rc = enc_pcm_up(e, h_pcm, NB))) return rc;
    rc = encode_dev_any(who, e, mode, p0, p1, h_rate ? e->d_rate : nullptr, false, e->d_pcm, nullptr, nBlocks, e->d_out, e->d_bits, e->d_wc, e->d_cplx, nullptr,
                        h_slots != nullptr, e->subSlots, n);
    return rc ? rc : enc_results_down(e, e->d_out, e->d_bits, NB, NB, h_out, h_bits, h_wc, h_cplx);
}
extern "C" int ulcx_encode_host(ulcx_encoder *e, int mode, float p0, float p1, const float *h_pcm, int nBlocks,
                                uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx) {
    const char *who = "ulcx_encode_host";
    if (enc_args_bad(who, e, h_pcm, h_out && h_bits, nBlocks)) return ULCX_ERR_ARG;
    if (!mode_ok(mode)) return refuse(who, "bad mode");
    return encode_host_any(who, e, mode, p0, p1, nullptr, h_pcm, nBlocks, h_out, h_bits, h_wc, h_cplx);
}
extern "C" int ulcx_encode_host_rates(ulcx_encoder *e, const ulcx_rate *h_rate, const float *h_pcm, int nBlocks,
                                      uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx) {
    const char *who = "ulcx_encode_host_rates";
    if (enc_args_bad(who, e, h_pcm, h_out && h_bits && h_rate, nBlocks)) return ULCX_ERR_ARG;
    if (rate_table_bad(who, "invalid entry for stream", h_rate, e->B)) return ULCX_ERR_ARG;          // ulcEncodeTool.c:43-50, before any device work
    return encode_host_any(who, e, 0, 0.0f, 0.0f, h_rate, h_pcm, nBlocks, h_out, h_bits, h_wc, h_cplx);
}
extern "C" int ulcx_encode_host_subset(ulcx_encoder *e, const int32_t *h_slots, int n, int mode, float p0, float p1, const ulcx_rate *h_rate, const float *h_pcm, int nBlocks,
                                       uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx) {
    const char *who = "ulcx_encode_host_subset";
    if (enc_args_bad(who, e, h_pcm, h_out && h_bits, nBlocks) || slots_host_bad(who, h_slots, n, e->B)) return ULCX_ERR_ARG;
    if (!h_rate && !mode_ok(mode)) return refuse(who, "bad mode");
    if (h_rate && rate_table_bad(who, "invalid entry for row", h_rate, n)) return ULCX_ERR_ARG;
    return encode_host_any(who, e, mode, p0, p1, h_rate, h_pcm, nBlocks, h_out, h_bits, h_wc, h_cplx, h_slots, n);
}

// The ladder's host-pointer form: every rung validated first (tables as ulcx_encode_host_rates validates its own, a scalar
// rung's parameters by the same rule), then input and tables up, one call on the null stream, [R][B][K] results down.
// Its slots and sizes have staging of their own, [ladRungs][B][maxK], grown to the largest ladder seen.
extern "C" int ulcx_encode_host_ladder(ulcx_encoder *e, const ulcx_rung *rungs, int nRungs, const float *h_pcm, int nBlocks,
                                       uint8_t *h_out, int32_t *h_bits, int32_t *h_wc, float *h_cplx) {
    const char *who = "ulcx_encode_host_ladder";
    if (ladder_bad(who, rungs, nRungs) || enc_args_bad(who, e, h_pcm, h_out && h_bits, nBlocks)) return ULCX_ERR_ARG;
    for (int r = 0; r < nRungs; r++) {
        char what[64];
        snprintf(what, sizeof(what), "rung %d: %s", r, rungs[r].rate ? "invalid setting for stream" : "invalid setting, mode");
        if (rungs[r].rate ? rate_table_bad(who, what, rungs[r].rate, e->B) : rate_entry_bad(who, what, rungs[r].mode, rungs[r].param0, rungs[r].param1)) return ULCX_ERR_ARG;
    }
    CKR(hipSetDevice(e->device));
    const size_t nBlk = (size_t)e->B * e->maxK, NB = (size_t)e->B * nBlocks;
    int rc = host_staging(e, true);
    if (!rc && e->ladRungs < nRungs) {
        e->ladRungs = 0;
        rc = dregrow(e->allocs, &e->ladOut, (size_t)nRungs * nBlk * e->ctx.slot, false);
        if (!rc) rc = dregrow(e->allocs, &e->ladBits, (size_t)nRungs * nBlk, false);
        if (!rc) e->ladRungs = nRungs;
    }
    if (!rc && !e->ladRate) rc = dalloc(e->allocs, &e->ladRate, (size_t)ULCX_MAX_RUNGS * e->B, false);
    if (rc) return rc;
    ulcx_rung dev[ULCX_MAX_RUNGS];
    for (int r = 0; r < nRungs; r++) {
        dev[r] = rungs[r];
        if (rungs[r].rate) {
            dev[r].rate = e->ladRate + (size_t)r * e->B;
            CKR(hipMemcpy((void *)dev[r].rate, rungs[r].rate, sizeof(ulcx_rate) * (size_t)e->B, hipMemcpyHostToDevice));
        }
    }
    if ((rc = enc_pcm_up(e, h_pcm, NB))) return rc;
    rc = encode_ladder_any(who, e, dev, nRungs, e->d_pcm, nullptr, nBlocks, e->ladOut, e->ladBits, e->d_wc, e->d_cplx, nullptr);
    return rc ? rc : enc_results_down(e, e->ladOut, e->ladBits, (size_t)nRungs * NB, NB, h_out, h_bits, h_wc, h_cplx);
}

// ---- clips (include/ulc_amd.h section 3): rows are whole clips in samples, channels-first; the output is a resident corpus.
// Per chunk of maxBlocksPerCall blocks: k_clip_stage into the object's staging, the plain call's launch sequence with c.B = n on
// the shadow state (reset in front of the first chunk, never scattered back) into the object's slots and sizes, k_clip_append,
// then the two kernels of ulcx_index_slots_dev on the masked sizes.  Everything on the caller's stream.
// ulcx_encode_clips_ladder_*: the same chunks with the ladder's launch sequence (nRungs contexts, rung r into its own part of
// the slots and sizes), the append and the index over nRungs * n files; ULCX_RUNG_AUTO rungs: an analysis pass over the same
// chunks in front, k_clip_cplx_sum behind each of them, k_clip_auto behind the last.
extern "C" int ulcx_clip_blocks(int BlockSize, int nSamples) {
    if (!validate(1, BlockSize) || nSamples < 1) return 0;
    return (int)(((long long)nSamples + BlockSize - 1) / BlockSize) + 2;          // cli/ulcx_tool.c:196 = ulcEncodeTool.c:93-98
}
// the checks every clips entry makes, device or host pointers: the arguments, then (behind the device forms' alignment checks)
// the objects - every other refusal needs none
static int clips_rows_bad(const char *who, int n, const void *pcm, int nSamples) {
    if (!pcm) { refuse(who, "bad argument (a NULL pointer)"); return 1; }
    if (nSamples < 1) { refuse(who, "bad argument (nSamples %d)", nSamples); return 1; }
    if (n < 1) { refuse(who, "bad argument (n %d)", n); return 1; }
    return 0;
}
static int clips_args_bad(const char *who, int n, const void *pcm, int nSamples,
                          const void *payload, long long payloadStride, const void *payloadBytes, const void *index, int indexStride, const void *indexBlocks) {
    if (!pcm || !payload || !payloadBytes || !index || !indexBlocks) { refuse(who, "bad argument (a NULL pointer)"); return 1; }
    if (nSamples < 1) { refuse(who, "bad argument (nSamples %d)", nSamples); return 1; }
    if (indexStride < 2 || payloadStride < 1) { refuse(who, "bad argument (payloadStride %lld, indexStride %d)", payloadStride, indexStride); return 1; }
    if (n < 1) { refuse(who, "bad argument (n %d)", n); return 1; }
    return 0;
}
// The setting(s) of a clips call.  The plain and _spectra entries hand the body one rung made of their own arguments
// (ladder == false: "bad mode" as ever); the ladder entries hand it the caller's rungs, checked as ulcx_encode_dev_ladder
// checks its own except that `reserved` may be ULCX_RUNG_AUTO - on a table rung, or on a scalar rung of mode CBR or ABR
// whose param0 is a rate (finite, > 0: it becomes RateKbps of a table entry, where a negative value would read as VBR).
static ulcx_rung clip_rung(int mode, float p0, float p1, const ulcx_rate *rate) { const ulcx_rung g = { mode, p0, p1, 0, rate }; return g; }
static bool rung_auto(const ulcx_rung &g) { return (g.reserved & ULCX_RUNG_AUTO) != 0; }
static int clips_setting_bad(const char *who, const ulcx_rung *rungs, int nRungs, bool ladder) {
    if (!ladder) {
        if (!rungs[0].rate && !mode_ok(rungs[0].mode)) { refuse(who, "bad mode"); return 1; }
        return 0;
    }
    if (!rungs || nRungs < 1 || nRungs > ULCX_MAX_RUNGS) { refuse(who, "nRungs %d not in 1 .. %d (or no rungs)", nRungs, ULCX_MAX_RUNGS); return 1; }
    for (int r = 0; r < nRungs; r++) {
        const ulcx_rung &g = rungs[r];
        if (g.reserved & ~ULCX_RUNG_AUTO) { refuse(who, "rung %d: reserved %d is neither 0 nor ULCX_RUNG_AUTO", r, (int)g.reserved); return 1; }
        if (!g.rate && !mode_ok(g.mode)) { refuse(who, "rung %d: bad mode %d", r, (int)g.mode); return 1; }
        if (!rung_auto(g) || g.rate) continue;
        if (g.mode == ULCX_MODE_VBR) { refuse(who, "rung %d: ULCX_RUNG_AUTO on a VBR rung (it needs a rate: mode CBR or ABR)", r); return 1; }
        if (!(isfinite(g.param0) && g.param0 > 0.0f)) { refuse(who, "rung %d: ULCX_RUNG_AUTO with RateKbps %g", r, (double)g.param0); return 1; }
    }
    return 0;
}
// the call's files (rows x rungs) and their index entries: what ulcx_index_slots_dev takes in one call (index_rows_any), and
// a file count that is an int.  It needs no object, so it stands in front of the object checks.
static int clips_files_bad(const char *who, long long nFiles, int indexStride) {
    if (nFiles <= 0x7FFFFFFFLL && nFiles * indexStride <= (0x7FFFFFFFLL << 8)) return 0;
    refuse(who, "%lld rows of %d entries are more than one call takes", nFiles, indexStride);
    return 1;
}
// dec == NULL passes with needDec false: the analysis forms have no decoder
static int clips_objects_bad(const char *who, const ulcx_encoder *e, const ulcx_decoder *dec, int n, bool needDec = true) {
    if (!e) { refuse(who, "no encoder"); return 1; }
    if (needDec && !dec) { refuse(who, "no decoder"); return 1; }
    if (n > e->B) { refuse(who, "bad argument (n %d: a call takes 1 .. nStreams = %d rows)", n, e->B); return 1; }
    if (needDec && (dec->C != e->C || dec->BS != e->BS || dec->device != e->device)) {
        refuse(who, "the decoder (%d x %d on device %d) is not of the encoder's geometry and device (%d x %d on %d)", dec->BS, dec->C, dec->device, e->BS, e->C, e->device);
        return 1;
    }
    return 0;
}
// The tap of ulcx_analyse_clips_* / ulcx_encode_clips_spectra_*: the caller's planes, device or host pointers.  on == false: the
// plain clips call.
struct ClipSpec { bool on = false; int nBlocks = 0, flags = 0; float *coef = nullptr; int32_t *wc = nullptr; float *cplx = nullptr; };
static int clip_spec_bad(const char *who, const ClipSpec &sp) {
    if (!sp.on) return 0;
    if (!sp.coef) { refuse(who, "bad argument (no coefficient planes)"); return 1; }
    if (sp.nBlocks < 1) { refuse(who, "bad argument (nBlocks %d)", sp.nBlocks); return 1; }
    if (sp.flags & ~ULCX_SPECTRA_LR) { refuse(who, "bad flags 0x%x", (unsigned)sp.flags); return 1; }
    return 0;
}
// nOutRungs: slots and sizes for that many rungs (0: the analysis forms write none), grown to the largest count seen as
// ulcx_encode_host_ladder's staging is; withSpec: the chunk's window codes and complexities; withAuto: the sums and tables of
// ULCX_RUNG_AUTO rungs
static int clips_staging(ulcx_encoder *e, int nOutRungs, bool withSpec, bool withAuto) {
    const size_t nBlk = (size_t)e->B * e->maxK;
    int rc = enc_shadow(e);
    if (!rc && !e->clipPcm) rc = dalloc(e->allocs, &e->clipPcm, nBlk * (size_t)e->C * e->BS, false);
    if (!rc && e->clipRungs < nOutRungs) {
        // the larger pair first, the smaller one freed behind it: a failed allocation leaves the staging the object had
        uint8_t *out = nullptr; int32_t *bits = nullptr;
        rc = dalloc(e->allocs, &out, (size_t)nOutRungs * nBlk * e->ctx.slot, false);
        if (!rc) rc = dalloc(e->allocs, &bits, (size_t)nOutRungs * nBlk, false);
        if (rc) { dfree(e->allocs, &out); dfree(e->allocs, &bits); return rc; }
        dfree(e->allocs, &e->clipOut); dfree(e->allocs, &e->clipBits);
        e->clipOut = out; e->clipBits = bits; e->clipRungs = nOutRungs;
    }
    if (!rc && withSpec && !e->clipWc) rc = dalloc(e->allocs, &e->clipWc, nBlk, false);
    if (!rc && withSpec && !e->clipCplx) rc = dalloc(e->allocs, &e->clipCplx, nBlk, false);
    if (!rc && withAuto && !e->clipSum) rc = dalloc(e->allocs, &e->clipSum, (size_t)e->B, false);
    if (!rc && withAuto && !e->clipRate) rc = dalloc(e->allocs, &e->clipRate, (size_t)ULCX_MAX_RUNGS * e->B, false);
    return rc;
}
// The body of the clips families.  rungs: the call's settings, file r * n + i being row i under rung r (ladder == false: the one
// rung a plain, _spectra or analysis entry made of its arguments).  chunkSamples: the longest row as far as the caller knows it
// (the _dev forms: nSamples) - the chunks stop behind its last block.  analyse: ulcx_analyse_clips_* - no rate, decoder or
// corpus, the analysis launch sequence per chunk.  sp.on: k_clip_spec behind every chunk's launch sequence, which then writes
// the chunk's window codes and complexities into the object's staging; plane blocks behind the last chunk are one more launch of
// it with an empty chunk.  A ULCX_RUNG_AUTO rung: the chunks run twice from the reset shadow state - an analysis pass whose
// complexities go into the rows' ordered sums, k_clip_auto, then the encode pass with the resolved tables in the AUTO rungs' place.
static int encode_clips_any(const char *who, ulcx_encoder *e, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs, bool ladder,
                            const float *d_pcm, const int16_t *d_pcm16, const int32_t *d_len, int nSamples, int chunkSamples,
                            uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock,
                            ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, float *d_avg, void *hipStream,
                            bool analyse = false, const ClipSpec &sp = ClipSpec()) {
    const void *pcm = d_pcm ? (const void *)d_pcm : d_pcm16;
    if (analyse ? clips_rows_bad(who, n, pcm, nSamples)
                : (clips_args_bad(who, n, pcm, nSamples, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks) ||
                   clips_setting_bad(who, rungs, nRungs, ladder))) return ULCX_ERR_ARG;
    if (clip_spec_bad(who, sp)) return ULCX_ERR_ARG;
    // (a plane starts at any sample: the staging kernel uses wider loads only where the address allows them)
    if (misaligned(who, "d_pcm", d_pcm, (int)sizeof(float)) || misaligned(who, "d_pcm16", d_pcm16, (int)sizeof(int16_t))) return ULCX_ERR_ARG;
    for (int r = 0; r < nRungs; r++) if (misaligned(who, ladder ? "a rung's rate table" : "d_rate", rungs[r].rate, ULCX_ALIGN_RATE)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_len", d_len, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_maxBlock", d_maxBlock, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) || misaligned(who, "d_indexBlocks", d_indexBlocks, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_avg", d_avg, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_coef", sp.coef, ULCX_ALIGN_PCM) || misaligned(who, "d_wc", sp.wc, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_cplx", sp.cplx, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    const long long nFiles = (long long)nRungs * n;
    if (!analyse && clips_files_bad(who, nFiles, indexStride)) return ULCX_ERR_ARG;
    if (clips_objects_bad(who, e, dec, n, !analyse)) return ULCX_ERR_ARG;
    bool anyAuto = false;
    for (int r = 0; r < nRungs; r++) anyAuto = anyAuto || rung_auto(rungs[r]);
    CKR(hipSetDevice(e->device));
    int rc = clips_staging(e, analyse ? 0 : nRungs, sp.on || anyAuto, anyAuto);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hipStream;
    const int total = ulcx_clip_blocks(e->BS, chunkSamples);
    const int lr = sp.flags & ULCX_SPECTRA_LR;
    ulcx_rung eff[ULCX_MAX_RUNGS];                                 // the rungs the encode pass runs: AUTO ones as their resolved tables
    for (int r = 0; r < nRungs; r++) eff[r] = rungs[r];
    int K = 0;
    // One pass over the call's chunks from the reset shadow state.  an: the analysis launch sequence; pre: the pass in front of
    // an encode with AUTO rungs (the sums instead of the tap).
    auto pass = [&](bool an, bool pre) -> int {
        const bool tap = sp.on && !pre;
        // (an analysis pass has no byte counts: the begin kernel's zeros go to the window-code staging, which every chunk rewrites)
        int rp = ulcx_clips_begin_launch(e->subHist, e->subWcs, n, e->C, e->BS, an ? n : (int)nFiles, an ? e->clipWc : d_payloadBytes, pre ? nullptr : d_maxBlock,
                                         pre ? e->clipSum : nullptr, st);
        if (rp) return rp;
        if (!an && (rp = ulcx_index_begin_launch((int)nFiles, d_index, indexStride, d_indexBlocks, st))) return rp;
        for (int k0 = 0; k0 < total; k0 += K) {
            K = total - k0 < e->maxK ? total - k0 : e->maxK;
            if ((rp = ulcx_clips_stage_launch(d_pcm, d_pcm16, d_len, nSamples, n, e->C, e->BS, k0, K, e->clipPcm, st))) return rp;
            UlcxEncCtx cs[ULCX_MAX_RUNGS];
            const int nc = an ? 1 : nRungs;
            for (int r = 0; r < nc; r++) {
                UlcxEncCtx &c = cs[r];
                c = an ? enc_call_ctx(e, ULCX_MODE_VBR, 100.0f, 0.0f, nullptr, e->clipPcm, nullptr, K)
                       : enc_call_ctx(e, eff[r].mode, eff[r].param0, eff[r].param1, eff[r].rate, e->clipPcm, nullptr, K);
                if (!an) { c.out = e->clipOut + (size_t)r * n * K * c.slot; c.bits = e->clipBits + (size_t)r * n * K; }
                if (!r && (tap || pre)) { c.wcOut = e->clipWc; c.cplxOut = e->clipCplx; }
                c.B = n; c.hist = e->subHist; c.wcs = e->subWcs;
            }
            if (an) rp = ulcx_analyse_launch(cs[0], st, e->timing ? e->ev : nullptr, enc_aux(e, K), e->analyseKxf);
            else rp = ulcx_enc_launch_ladder(cs, nRungs, st, e->timing ? e->ev : nullptr, enc_aux(e, K));
            if (rp) return rp;
            if (tap && (rp = ulcx_clips_spec_launch(n, K, k0, sp.nBlocks - k0 < K ? sp.nBlocks - k0 : K, e->C, e->BS, nSamples, d_len, cs[0].coef, e->clipWc, e->clipCplx,
                                                    sp.nBlocks, lr, sp.coef, sp.wc, sp.cplx, st))) return rp;
            if (pre && (rp = ulcx_clips_cplx_sum_launch(n, K, k0, e->BS, nSamples, d_len, e->clipCplx, e->clipSum, st))) return rp;
            if (an) continue;
            const int slot = cs[0].slot;
            if ((rp = ulcx_clips_append_launch(n, nRungs, K, k0, e->BS, nSamples, d_len, slot, e->clipOut, e->clipBits, d_payload, payloadStride, d_payloadBytes, d_maxBlock,
                                               indexStride, d_indexBlocks, st))) return rp;
            UlcxDecCtx dc = dec->ctx;
            dc.in = e->clipOut; dc.slot = slot; dc.inBytes = nFiles * K * slot;
            if ((rp = ulcx_index_slots_launch(dc, (int)nFiles, K, e->clipBits, d_index, indexStride, d_indexBlocks, st))) return rp;
        }
        return ULCX_OK;
    };
    if (anyAuto) {
        rc = pass(true, true);
        if (rc == ULCX_OK) rc = ulcx_clips_auto_launch(n, e->BS, nSamples, d_len, e->clipSum, rungs, nRungs, e->clipRate, d_avg, st);
        for (int r = 0; r < nRungs; r++) if (rung_auto(rungs[r])) { eff[r].rate = e->clipRate + (size_t)r * n; eff[r].reserved = 0; }
    }
    if (rc == ULCX_OK) rc = pass(analyse, false);
    if (sp.on && rc == ULCX_OK && total < sp.nBlocks)
        rc = ulcx_clips_spec_launch(n, 0, total, sp.nBlocks - total, e->C, e->BS, nSamples, d_len, e->ctx.coef, e->clipWc, e->clipCplx,
                                    sp.nBlocks, lr, sp.coef, sp.wc, sp.cplx, st);
    return K ? enc_call_done(e, rc, K, analyse, analyse ? 0 : nRungs) : rc;
}
static ClipSpec clip_spec(int nBlocks, int flags, float *coef, int32_t *wc, float *cplx) {
    ClipSpec sp; sp.on = true; sp.nBlocks = nBlocks; sp.flags = flags; sp.coef = coef; sp.wc = wc; sp.cplx = cplx;
    return sp;
}
extern "C" int ulcx_encode_clips_dev(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *d_rate,
                                     const float *d_pcm, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes,
                                     int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, void *hipStream) {
    const ulcx_rung g = clip_rung(mode, p0, p1, d_rate);
    return encode_clips_any("ulcx_encode_clips_dev", e, dec, n, &g, 1, false, d_pcm, nullptr, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, nullptr, hipStream);
}
extern "C" int ulcx_encode_clips_dev_pcm16(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *d_rate,
                                           const int16_t *d_pcm16, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes,
                                           int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, void *hipStream) {
    const ulcx_rung g = clip_rung(mode, p0, p1, d_rate);
    return encode_clips_any("ulcx_encode_clips_dev_pcm16", e, dec, n, &g, 1, false, nullptr, d_pcm16, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, nullptr, hipStream);
}
extern "C" int ulcx_encode_clips_ladder_dev(ulcx_encoder *e, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                            const float *d_pcm, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes,
                                            int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks, float *d_avg, void *hipStream) {
    return encode_clips_any("ulcx_encode_clips_ladder_dev", e, dec, n, rungs, nRungs, true, d_pcm, nullptr, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, d_avg, hipStream);
}
extern "C" int ulcx_encode_clips_ladder_dev_pcm16(ulcx_encoder *e, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                                  const int16_t *d_pcm16, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride,
                                                  int32_t *d_payloadBytes, int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks,
                                                  float *d_avg, void *hipStream) {
    return encode_clips_any("ulcx_encode_clips_ladder_dev_pcm16", e, dec, n, rungs, nRungs, true, nullptr, d_pcm16, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, d_avg, hipStream);
}
extern "C" int ulcx_encode_clips_spectra_dev(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *d_rate,
                                             const float *d_pcm, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes,
                                             int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks,
                                             int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream) {
    const ulcx_rung g = clip_rung(mode, p0, p1, d_rate);
    return encode_clips_any("ulcx_encode_clips_spectra_dev", e, dec, n, &g, 1, false, d_pcm, nullptr, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, nullptr, hipStream, false, clip_spec(nBlocks, flags, d_coef, d_wc, d_cplx));
}
extern "C" int ulcx_encode_clips_spectra_dev_pcm16(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *d_rate,
                                                   const int16_t *d_pcm16, const int32_t *d_len, int nSamples, uint8_t *d_payload, long long payloadStride,
                                                   int32_t *d_payloadBytes, int32_t *d_maxBlock, ulcx_index_entry *d_index, int indexStride, int32_t *d_indexBlocks,
                                                   int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream) {
    const ulcx_rung g = clip_rung(mode, p0, p1, d_rate);
    return encode_clips_any("ulcx_encode_clips_spectra_dev_pcm16", e, dec, n, &g, 1, false, nullptr, d_pcm16, d_len, nSamples, nSamples, d_payload, payloadStride,
                            d_payloadBytes, d_maxBlock, d_index, indexStride, d_indexBlocks, nullptr, hipStream, false, clip_spec(nBlocks, flags, d_coef, d_wc, d_cplx));
}
static const ulcx_rung kNoRung = { ULCX_MODE_VBR, 100.0f, 0.0f, 0, nullptr };      // the analysis forms: no setting
extern "C" int ulcx_analyse_clips_dev(ulcx_encoder *e, int n, const float *d_pcm, const int32_t *d_len, int nSamples,
                                      int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_clips_any("ulcx_analyse_clips_dev", e, nullptr, n, &kNoRung, 1, false, d_pcm, nullptr, d_len, nSamples, nSamples, nullptr, 0,
                            nullptr, nullptr, nullptr, 0, nullptr, nullptr, hipStream, true, clip_spec(nBlocks, flags, d_coef, d_wc, d_cplx));
}
extern "C" int ulcx_analyse_clips_dev_pcm16(ulcx_encoder *e, int n, const int16_t *d_pcm16, const int32_t *d_len, int nSamples,
                                            int nBlocks, int flags, float *d_coef, int32_t *d_wc, float *d_cplx, void *hipStream) {
    return encode_clips_any("ulcx_analyse_clips_dev_pcm16", e, nullptr, n, &kNoRung, 1, false, nullptr, d_pcm16, d_len, nSamples, nSamples, nullptr, 0,
                            nullptr, nullptr, nullptr, 0, nullptr, nullptr, hipStream, true, clip_spec(nBlocks, flags, d_coef, d_wc, d_cplx));
}
// The host forms: every check first, then everything up into buffers of the call's own, the body on the null stream with the
// longest row's length, one synchronisation, and down: counts, index, and of every payload the bytes that are defined (the
// nRungs * n files of a ladder form; its averages where an AUTO rung wrote them); the planes of a spectra form in full.
// analyse: no rate, decoder or corpus.  A rung's table is validated by the one validator (rate_entry_bad); the ladder form also
// validates a scalar rung's parameters as ulcx_encode_host_ladder does, and refuses AUTO on a table row that is VBR.
static int encode_clips_host_any(const char *who, ulcx_encoder *e, ulcx_decoder *dec, bool analyse, int n, const ulcx_rung *rungs, int nRungs, bool ladder,
                                 const float *h_pcm, const int32_t *h_len, int nSamples, uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes,
                                 int32_t *h_maxBlock, ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks, float *h_avg, const ClipSpec &sp) {
    if ((analyse ? clips_rows_bad(who, n, h_pcm, nSamples)
                 : (clips_args_bad(who, n, h_pcm, nSamples, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks) ||
                    clips_setting_bad(who, rungs, nRungs, ladder))) ||
        clip_spec_bad(who, sp) || (!analyse && clips_files_bad(who, (long long)nRungs * n, indexStride)) ||
        clips_objects_bad(who, e, dec, n, !analyse)) return ULCX_ERR_ARG;
    int longest = h_len ? 0 : nSamples;
    for (int i = 0; h_len && i < n; i++) {
        if (h_len[i] < 0) return refuse(who, "row %d has %d samples", i, (int)h_len[i]);
        const int l = h_len[i] > nSamples ? nSamples : h_len[i];
        if (l > longest) longest = l;
    }
    bool anyAuto = false;
    for (int r = 0; r < nRungs && !analyse; r++) {
        const ulcx_rung &g = rungs[r];
        char what[64];
        if (!ladder) snprintf(what, sizeof(what), "invalid entry for row");
        else snprintf(what, sizeof(what), "rung %d: %s", r, g.rate ? "invalid entry for row" : "invalid setting, mode");
        if (g.rate ? rate_table_bad(who, what, g.rate, n) : (ladder && rate_entry_bad(who, what, g.mode, g.param0, rung_auto(g) ? 0.0f : g.param1))) return ULCX_ERR_ARG;
        if (!rung_auto(g)) continue;
        anyAuto = true;
        for (int i = 0; g.rate && i < n; i++)
            if (g.rate[i].RateKbps < 0.0f) return refuse(who, "rung %d: ULCX_RUNG_AUTO on row %d, a VBR row (RateKbps %g)", r, i, (double)g.rate[i].RateKbps);
    }
    const long long nFiles = (long long)nRungs * n;
    CKR(hipSetDevice(e->device));
    const size_t nF = (size_t)nFiles, nPcm = (size_t)n * e->C * (size_t)nSamples, nEnt = nF * (size_t)indexStride;
    const size_t nPlane = (size_t)n * (size_t)sp.nBlocks, nCoef = nPlane * (size_t)e->C * e->BS;
    DevTmp t; float *dpcm = nullptr, *davg = nullptr; int32_t *dlen = nullptr, *dbytes = nullptr, *dmax = nullptr, *dcnt = nullptr;
    uint8_t *dpay = nullptr; ulcx_index_entry *di = nullptr;
    ClipSpec dsp = sp;
    ulcx_rung dev[ULCX_MAX_RUNGS];
    CKR(t.get(&dpcm, sizeof(float) * nPcm));
    if (!analyse) {
        CKR(t.get(&dpay, nF * (size_t)payloadStride));
        CKR(t.get(&dbytes, sizeof(int32_t) * nF)); CKR(t.get(&dmax, sizeof(int32_t) * nF)); CKR(t.get(&dcnt, sizeof(int32_t) * nF));
        CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt));
    }
    if (sp.on) {
        CKR(t.get(&dsp.coef, sizeof(float) * nCoef));
        if (sp.wc) CKR(t.get(&dsp.wc, sizeof(int32_t) * nPlane));
        if (sp.cplx) CKR(t.get(&dsp.cplx, sizeof(float) * nPlane));
    }
    CKR(hipMemcpy(dpcm, h_pcm, sizeof(float) * nPcm, hipMemcpyHostToDevice));
    if (h_len) { CKR(t.get(&dlen, sizeof(int32_t) * n)); CKR(hipMemcpy(dlen, h_len, sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
    for (int r = 0; r < nRungs; r++) {
        dev[r] = rungs[r];
        if (!rungs[r].rate) continue;
        ulcx_rate *drate = nullptr;
        CKR(t.get(&drate, sizeof(ulcx_rate) * n)); CKR(hipMemcpy(drate, rungs[r].rate, sizeof(ulcx_rate) * n, hipMemcpyHostToDevice));
        dev[r].rate = drate;
    }
    if (anyAuto && h_avg) CKR(t.get(&davg, sizeof(float) * n));
    const int rc = encode_clips_any(who, e, dec, n, dev, nRungs, ladder, dpcm, nullptr, dlen, nSamples, longest, dpay, payloadStride, dbytes, dmax, di, indexStride, dcnt, davg,
                                    nullptr, analyse, dsp);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    if (sp.on) {
        CKR(hipMemcpy(sp.coef, dsp.coef, sizeof(float) * nCoef, hipMemcpyDeviceToHost));
        if (sp.wc) CKR(hipMemcpy(sp.wc, dsp.wc, sizeof(int32_t) * nPlane, hipMemcpyDeviceToHost));
        if (sp.cplx) CKR(hipMemcpy(sp.cplx, dsp.cplx, sizeof(float) * nPlane, hipMemcpyDeviceToHost));
    }
    if (analyse) return ULCX_OK;
    CKR(hipMemcpy(h_payloadBytes, dbytes, sizeof(int32_t) * nF, hipMemcpyDeviceToHost));
    if (h_maxBlock) CKR(hipMemcpy(h_maxBlock, dmax, sizeof(int32_t) * nF, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_indexBlocks, dcnt, sizeof(int32_t) * nF, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_index, di, sizeof(ulcx_index_entry) * nEnt, hipMemcpyDeviceToHost));
    if (davg) CKR(hipMemcpy(h_avg, davg, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (size_t f = 0; f < nF; f++)
        if (h_payloadBytes[f] > 0) CKR(hipMemcpy(h_payload + f * (size_t)payloadStride, dpay + f * (size_t)payloadStride, (size_t)h_payloadBytes[f], hipMemcpyDeviceToHost));
    return ULCX_OK;
}
extern "C" int ulcx_encode_clips_host(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *h_rate,
                                      const float *h_pcm, const int32_t *h_len, int nSamples, uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes,
                                      int32_t *h_maxBlock, ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks) {
    const ulcx_rung g = clip_rung(mode, p0, p1, h_rate);
    return encode_clips_host_any("ulcx_encode_clips_host", e, dec, false, n, &g, 1, false, h_pcm, h_len, nSamples, h_payload, payloadStride, h_payloadBytes,
                                 h_maxBlock, h_index, indexStride, h_indexBlocks, nullptr, ClipSpec());
}
extern "C" int ulcx_encode_clips_ladder_host(ulcx_encoder *e, ulcx_decoder *dec, int n, const ulcx_rung *rungs, int nRungs,
                                             const float *h_pcm, const int32_t *h_len, int nSamples, uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes,
                                             int32_t *h_maxBlock, ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks, float *h_avg) {
    return encode_clips_host_any("ulcx_encode_clips_ladder_host", e, dec, false, n, rungs, nRungs, true, h_pcm, h_len, nSamples, h_payload, payloadStride, h_payloadBytes,
                                 h_maxBlock, h_index, indexStride, h_indexBlocks, h_avg, ClipSpec());
}
extern "C" int ulcx_encode_clips_spectra_host(ulcx_encoder *e, ulcx_decoder *dec, int n, int mode, float p0, float p1, const ulcx_rate *h_rate,
                                              const float *h_pcm, const int32_t *h_len, int nSamples, uint8_t *h_payload, long long payloadStride, int32_t *h_payloadBytes,
                                              int32_t *h_maxBlock, ulcx_index_entry *h_index, int indexStride, int32_t *h_indexBlocks,
                                              int nBlocks, int flags, float *h_coef, int32_t *h_wc, float *h_cplx) {
    const ulcx_rung g = clip_rung(mode, p0, p1, h_rate);
    return encode_clips_host_any("ulcx_encode_clips_spectra_host", e, dec, false, n, &g, 1, false, h_pcm, h_len, nSamples, h_payload, payloadStride, h_payloadBytes,
                                 h_maxBlock, h_index, indexStride, h_indexBlocks, nullptr, clip_spec(nBlocks, flags, h_coef, h_wc, h_cplx));
}
extern "C" int ulcx_analyse_clips_host(ulcx_encoder *e, int n, const float *h_pcm, const int32_t *h_len, int nSamples,
                                       int nBlocks, int flags, float *h_coef, int32_t *h_wc, float *h_cplx) {
    return encode_clips_host_any("ulcx_analyse_clips_host", e, nullptr, true, n, &kNoRung, 1, false, h_pcm, h_len, nSamples, nullptr, 0, nullptr,
                                 nullptr, nullptr, 0, nullptr, nullptr, clip_spec(nBlocks, flags, h_coef, h_wc, h_cplx));
}

// ---- strided corpus -> ragged corpus (include/ulc_amd.h section 3): no object; two kernels of ulcx_clips.hip
static int corpus_ragged_bad(const char *who, int nFiles, const void *payload, long long payloadStride, const void *payloadBytes, const void *index, int indexStride,
                             const void *indexBlocks, const void *outPayload, long long payloadCap, const void *payloadOffs, const void *outIndex, long long indexCap,
                             const void *indexOffs, const void *outIndexBlocks, const void *need) {
    if (!payload || !payloadBytes || !index || !indexBlocks || !outPayload || !payloadOffs || !outIndex || !indexOffs || !outIndexBlocks || !need) {
        refuse(who, "bad argument (a NULL pointer)"); return 1;
    }
    if (nFiles < 1) { refuse(who, "bad argument (nFiles %d)", nFiles); return 1; }
    if (payloadStride < 1 || indexStride < 1) { refuse(who, "bad argument (payloadStride %lld, indexStride %d)", payloadStride, indexStride); return 1; }
    if (payloadCap < 0 || indexCap < 0) { refuse(who, "bad argument (payloadCap %lld, indexCap %lld)", payloadCap, indexCap); return 1; }
    return 0;
}
extern "C" int ulcx_corpus_ragged_dev(int device, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                      const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                      uint8_t *d_outPayload, long long payloadCap, int64_t *d_payloadOffs, ulcx_index_entry *d_outIndex, long long indexCap,
                                      int64_t *d_indexOffs, int32_t *d_outIndexBlocks, int64_t *d_need, void *hipStream) {
    const char *who = "ulcx_corpus_ragged_dev";
    if (corpus_ragged_bad(who, nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks, d_outPayload, payloadCap, d_payloadOffs,
                          d_outIndex, indexCap, d_indexOffs, d_outIndexBlocks, d_need)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_indexBlocks", d_indexBlocks, ULCX_ALIGN_WORD) || misaligned(who, "d_payloadOffs", d_payloadOffs, ULCX_ALIGN_OFFS) ||
        misaligned(who, "d_outIndex", d_outIndex, ULCX_ALIGN_WORD) || misaligned(who, "d_indexOffs", d_indexOffs, ULCX_ALIGN_OFFS) ||
        misaligned(who, "d_outIndexBlocks", d_outIndexBlocks, ULCX_ALIGN_WORD) || misaligned(who, "d_need", d_need, ULCX_ALIGN_OFFS)) return ULCX_ERR_ARG;
    const int rc = select_device(who, device);
    if (rc) return rc;
    return ulcx_corpus_ragged_launch(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks, d_outPayload, payloadCap, d_payloadOffs,
                                     d_outIndex, indexCap, d_indexOffs, d_outIndexBlocks, d_need, (hipStream_t)hipStream);
}
extern "C" int ulcx_corpus_ragged_host(int device, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                       const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                       uint8_t *h_outPayload, long long payloadCap, int64_t *h_payloadOffs, ulcx_index_entry *h_outIndex, long long indexCap,
                                       int64_t *h_indexOffs, int32_t *h_outIndexBlocks, int64_t *h_need) {
    const char *who = "ulcx_corpus_ragged_host";
    if (corpus_ragged_bad(who, nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks, h_outPayload, payloadCap, h_payloadOffs,
                          h_outIndex, indexCap, h_indexOffs, h_outIndexBlocks, h_need)) return ULCX_ERR_ARG;
    int rc = select_device(who, device);
    if (rc) return rc;
    const size_t F = (size_t)nFiles, nEnt = F * (size_t)indexStride;
    DevTmp t; uint8_t *dp = nullptr, *dop = nullptr; int32_t *dn = nullptr, *dcnt = nullptr, *docnt = nullptr; ulcx_index_entry *di = nullptr, *doi = nullptr;
    int64_t *dpo = nullptr, *dio = nullptr, *dneed = nullptr;
    CKR(t.get(&dp, F * (size_t)payloadStride)); CKR(t.get(&dn, sizeof(int32_t) * F)); CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt));
    CKR(t.get(&dcnt, sizeof(int32_t) * F)); CKR(t.get(&dop, (size_t)payloadCap)); CKR(t.get(&doi, sizeof(ulcx_index_entry) * (size_t)indexCap));
    CKR(t.get(&dpo, sizeof(int64_t) * (F + 1))); CKR(t.get(&dio, sizeof(int64_t) * (F + 1))); CKR(t.get(&docnt, sizeof(int32_t) * F)); CKR(t.get(&dneed, sizeof(int64_t) * 2));
    CKR(hipMemcpy(dp, h_payload, F * (size_t)payloadStride, hipMemcpyHostToDevice));
    CKR(hipMemcpy(dn, h_payloadBytes, sizeof(int32_t) * F, hipMemcpyHostToDevice));
    CKR(hipMemcpy(di, h_index, sizeof(ulcx_index_entry) * nEnt, hipMemcpyHostToDevice));
    CKR(hipMemcpy(dcnt, h_indexBlocks, sizeof(int32_t) * F, hipMemcpyHostToDevice));
    rc = ulcx_corpus_ragged_dev(device, nFiles, dp, payloadStride, dn, di, indexStride, dcnt, dop, payloadCap, dpo, doi, indexCap, dio, docnt, dneed, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_payloadOffs, dpo, sizeof(int64_t) * (F + 1), hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_indexOffs, dio, sizeof(int64_t) * (F + 1), hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_outIndexBlocks, docnt, sizeof(int32_t) * F, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_need, dneed, sizeof(int64_t) * 2, hipMemcpyDeviceToHost));
    if (h_payloadOffs[F] > 0) CKR(hipMemcpy(h_outPayload, dop, (size_t)h_payloadOffs[F], hipMemcpyDeviceToHost));
    if (h_indexOffs[F] > 0) CKR(hipMemcpy(h_outIndex, doi, sizeof(ulcx_index_entry) * (size_t)h_indexOffs[F], hipMemcpyDeviceToHost));
    return ULCX_OK;
}

// One block of one stream per call (the drop-in ABI): include/ulc_amd.h.  The launch sequence of ulcx_encode_dev - side
// streams and their event fork/joins included - is captured once into a graph together with the copies between the pinned
// staging buffers and the device; a call is then memcpy, one graph launch, one synchronisation, memcpy.
extern "C" int ulcx_encode_block1(ulcx_encoder *e, int mode, float p0, float p1, const float *h_pcm,
                                  uint8_t *h_out, int32_t *bits, float *cplx, int32_t stateOut[2], float transientFilter[3]) {
    const char *who = "ulcx_encode_block1";
    if (!e || !h_pcm || !h_out || e->B != 1 || e->maxK != 1) return refuse(who, "needs an encoder of one stream, one block per call");
    if (!mode_ok(mode)) return refuse(who, "bad mode");
    CKR(hipSetDevice(e->device));
    const size_t cb = (size_t)e->C * e->BS, slot = (size_t)e->ctx.slot;
    if (!e->b1Init) {
        int rc;
        if ((rc = host_staging(e, true))) return rc;                   // (one stream, one block per call)
        // (b1Init only once everything exists: a failed allocation leaves the call to be retried from scratch, never a
        //  later call copying into a null staging buffer)
        if (!e->b1.stream) CKR(hipStreamCreateWithFlags(&e->b1.stream, hipStreamNonBlocking));
        if (!e->pinIn) CKR(hipHostMalloc((void **)&e->pinIn, sizeof(float) * cb, hipHostMallocDefault));
        if (!e->pinOut) CKR(hipHostMalloc((void **)&e->pinOut, slot, hipHostMallocDefault));
        if (!e->pinMeta) CKR(hipHostMalloc((void **)&e->pinMeta, sizeof(*e->pinMeta), hipHostMallocDefault));
        e->b1Init = true;
        e->timing = false;                                 // (per-kernel events cannot be captured, and nobody reads them here)
    }
    auto enqueue = [&]() -> int {
        CKR(hipMemcpyAsync(e->d_pcm, e->pinIn, sizeof(float) * cb, hipMemcpyHostToDevice, e->b1.stream));
        int rc = encode_dev_any(who, e, mode, p0, p1, nullptr, false, e->d_pcm, nullptr, 1, e->d_out, e->d_bits, e->d_wc, e->d_cplx, e->b1.stream);
        if (rc) return rc;
        CKR(hipMemcpyAsync(e->pinOut, e->d_out, slot, hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta->bits, e->d_bits, sizeof(int32_t), hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta->wc, e->d_wc, sizeof(int32_t), hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta->cplx, e->d_cplx, sizeof(float), hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta->wcs, e->ctx.wcs, sizeof(UlcxWcState), hipMemcpyDeviceToHost, e->b1.stream));
        return ULCX_OK;
    };
    memcpy(e->pinIn, h_pcm, sizeof(float) * cb);
    if (e->b1.graphed && (e->b1Mode != mode || e->b1P0 != p0 || e->b1P1 != p1)) {         // the parameters are part of the captured kernels' arguments
        block1_drop(e->b1);
        // a caller whose parameters change from block to block (ULC_EncodeBlock_ABR: the reference's tool updates
        // AvgComplexity every block) would pay a capture + instantiate per call: after the second change, direct launches
        if (++e->b1Rekeys >= 2) e->b1.noGraph = true;
    }
    if (!e->b1.graphed) { e->b1Mode = mode; e->b1P0 = p0; e->b1P1 = p1; }                  // (what a capture in this call holds)
    { int rc = block1_run(e->b1, enqueue); if (rc) return rc; }
    const int32_t nb = e->pinMeta->bits;
    memcpy(h_out, e->pinOut, (nb > 0 && (size_t)(nb + 7) / 8 <= slot) ? (size_t)(nb + 7) / 8 : slot);
    if (bits) *bits = nb;
    if (cplx) *cplx = e->pinMeta->cplx;
    if (stateOut) { stateOut[0] = e->pinMeta->wcs.wcPrev; stateOut[1] = e->pinMeta->wcs.wcCur; }     // WindowCtrl of this block, NextWindowCtrl
    if (transientFilter) for (int i = 0; i < 3; i++) transientFilter[i] = e->pinMeta->wcs.tf[i];
    return ULCX_OK;
}

extern "C" int ulcx_encoder_debug_fetch(ulcx_encoder *e, int nBlocks, float *h_coef, float *h_noise, float *h_keys, uint8_t *h_keep, int32_t *h_nout) {
    const char *who = "ulcx_encoder_debug_fetch";
    if (!e || nBlocks < 1 || nBlocks > e->maxK) return refuse(who, "no encoder, or nBlocks out of range");
    if (e->lastAnalyse) return refuse(who, "the last call was an analysis call (no intermediates)");
    CKR(hipSetDevice(e->device));
    CKR(hipDeviceSynchronize());
    size_t NB = (size_t)e->B * nBlocks, cb = (size_t)e->C * e->BS;
    if (h_coef)  CKR(hipMemcpy(h_coef, e->ctx.coef, sizeof(float) * NB * cb, hipMemcpyDeviceToHost));
    if (h_noise) {
        // the {w, w*log} pairs (the reference's TransformNoise) are not an array of the pipeline any more: formed here, for the tap
        if (!e->ctx.npair) { int rc = dalloc(e->allocs, &e->ctx.npair, (size_t)e->B * e->maxK * cb, false); if (rc) return rc; }
        UlcxEncCtx c2 = e->ctx; c2.K = nBlocks;
        ulcx_enc_materialise_noise(c2, nullptr);
        CKR(hipDeviceSynchronize());
        CKR(hipMemcpy(h_noise, e->ctx.npair, sizeof(float) * NB * cb, hipMemcpyDeviceToHost));
    }
    if (h_keys) {
        if (!e->keysFinal) {                       // the pipeline never writes final keys back; materialise them for the tap
            UlcxEncCtx c2 = e->ctx; c2.K = nBlocks; c2.keyFinal = 0;
            ulcx_enc_finalize_keys(c2, nullptr);
            CKR(hipDeviceSynchronize());
            e->keysFinal = true;
        }
        CKR(hipMemcpy(h_keys, e->ctx.key, sizeof(float) * NB * cb, hipMemcpyDeviceToHost));
    }
    if (h_nout)  CKR(hipMemcpy(h_nout, e->ctx.nout, sizeof(int32_t) * NB, hipMemcpyDeviceToHost));
    if (h_keep) {
        std::vector<uint32_t> bits(NB * cb / 32);
        CKR(hipMemcpy(bits.data(), e->ctx.keep, sizeof(uint32_t) * bits.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < NB * cb; i++) h_keep[i] = (bits[i >> 5] >> (i & 31)) & 1;
    }
    return ULCX_OK;
}

extern "C" int ulcx_encoder_debug_force_exact(ulcx_encoder *e, int every) {
    if (!e || every < 0) return refuse("ulcx_encoder_debug_force_exact", "no encoder, or every < 0");
    e->ctx.forceFb = every;
    return ULCX_OK;
}
extern "C" int ulcx_encoder_last_fallbacks(ulcx_encoder *e) {
    if (!e) return refuse("ulcx_encoder_last_fallbacks", "no encoder");
    if (e->lastAnalyse) return 0;                                      // (an analysis call selects nothing)
    CKR(hipSetDevice(e->device));
    CKR(hipDeviceSynchronize());
    int n[2] = { 0, 0 };                                               // this call's (last rung's) count; a ladder call: the rungs in front of it
    CKR(hipMemcpy(n, e->ctx.fbCount, sizeof(n), hipMemcpyDeviceToHost));
    return n[0] + (e->lastRungs > 1 ? n[1] : 0);
}
// Test hooks: the wave writer's give-up bits of the last call's final pass (c.slow[0 .. B*K)), and the capacities it launches with.
// The capacities are enc_plan's (ulcx_enc.hip), restated over the same constants and the same LDS formula (ulcx_enc_dev.h): that
// translation unit holds kernels and is not rebuilt for a test hook.  tests/test_gpu_writer_tiers.py pins the values per geometry.
static void ulcx_enc_writer_plan(const UlcxEncCtx &c, int caps[3][3], int *haveMid, int *haveFull) {
    const WaveCaps capS = { WAVE_SK, WAVE_SZ, WAVE_SN }, capM = { 1024, 512, 4096 };
    WaveCaps capF = { (c.BS + 63) & ~63, ((c.BS / 2) + 63) & ~63, 4 * c.BS + 64 };
    while ((size_t)wavecaps_lds(capF) * 4 > 150 * 1024) { capF.k = (capF.k / 2 + 63) & ~63; capF.z = (capF.z / 2 + 63) & ~63; capF.nyb = capF.nyb / 2 + 32; }
    const WaveCaps t[3] = { capS, capM, capF };
    for (int i = 0; i < 3; i++) { caps[i][0] = t[i].k; caps[i][1] = t[i].z; caps[i][2] = t[i].nyb; }
    *haveFull = capF.k > capS.k;
    *haveMid = capM.k < capF.k;
}
extern "C" int ulcx_encoder_debug_writer_flags(ulcx_encoder *e, int nBlocks, int32_t *h_flags) {
    const char *who = "ulcx_encoder_debug_writer_flags";
    if (!e || !h_flags) return refuse(who, "no encoder, or no array");
    if (e->lastAnalyse) return refuse(who, "the last call was an analysis call (no writer ran)");
    if (e->lastRungs < 1 || nBlocks != e->lastK) return refuse(who, "nBlocks is not the last encode call's (or there was none)");
    CKR(hipSetDevice(e->device));
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_flags, e->ctx.slow, sizeof(int32_t) * (size_t)e->B * nBlocks, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
extern "C" int ulcx_encoder_debug_writer_plan(ulcx_encoder *e, int32_t plan[11]) {
    const char *who = "ulcx_encoder_debug_writer_plan";
    if (!e || !plan) return refuse(who, "no encoder, or no array");
    int caps[3][3], haveMid = 0, haveFull = 0;
    ulcx_enc_writer_plan(e->ctx, caps, &haveMid, &haveFull);
    for (int t = 0; t < 3; t++) for (int i = 0; i < 3; i++) plan[3 * t + i] = caps[t][i];
    plan[9] = haveMid; plan[10] = haveFull;
    return ULCX_OK;
}
// Test hook: what create decided for this object.  selPair and the heap's place are enc_plan's (ulcx_enc.hip), restated for the
// reason given at ulcx_enc_writer_plan.
extern "C" int ulcx_encoder_debug_plan(ulcx_encoder *e, int32_t plan[7]) {
    if (!e || !plan) return refuse("ulcx_encoder_debug_plan", "no encoder, or no array");
    const UlcxEncCtx &c = e->ctx;
    const size_t cb = (size_t)c.C * c.BS;
    plan[0] = c.barkRing; plan[1] = e->barkMost; plan[2] = c.useGapSums;
    plan[3] = (cb * 8 <= ULCX_HEAP_LDS_BYTES) ? 1 : 0;
    plan[4] = e->nsSlots; plan[5] = e->wcPipe;
    plan[6] = (cb / 64 == 128 && c.C == 2 && c.selPair) ? 1 : 0;
    return ULCX_OK;
}
// Test hook: where launch_front (ulcx_enc.hip) would cut a call of nBlocks - enc_aux's chunk count through ulcx_front_plan, the
// function the launch itself calls.
static_assert(ULCX_FRONT_PLAN_WORDS == 2 + (ULCX_XF_MAXCH + 1) + (ULCX_WC_MAXCH + 1), "include/ulc_amd.h: the words the hook may write");
extern "C" int ulcx_encoder_debug_front_plan(ulcx_encoder *e, int nBlocks, int32_t *out) {
    const char *who = "ulcx_encoder_debug_front_plan";
    if (!e || !out) return refuse(who, "no encoder, or no array");
    if (nBlocks < 1 || nBlocks > e->maxK) return refuse(who, "nBlocks out of range");
    const UlcxEncAux aux = enc_aux(e, nBlocks);
    const UlcxFrontPlan fp = ulcx_front_plan(nBlocks, aux.wcPipe, aux.wcSteps);
    int n = 0;
    out[n++] = fp.nCh; out[n++] = fp.nW;
    for (int j = 0; j <= fp.nCh; j++) out[n++] = fp.cut[j];
    for (int w = 0; w <= fp.nW; w++) out[n++] = fp.wcs[w];
    while (n < ULCX_FRONT_PLAN_WORDS) out[n++] = -1;
    return ULCX_OK;
}
extern "C" const char *ulcx_encoder_stage_name(int i) { return (i >= 0 && i < ULCX_ENC_STAGES_REPORTED) ? ulcx_enc_stage_names[i] : ""; }
extern "C" int ulcx_encoder_stage_ms(ulcx_encoder *e, float *ms, int maxStages) {
    if (!e || !e->evRecorded) return 0;
    int n = 0;
    for (int i = 0; i < ULCX_ENC_STAGES && i < maxStages; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, e->ev[i], e->ev[i + 1]) != hipSuccess) break;
        ms[n++] = (e->lastAnalyse && i > 6 && i < ULCX_ENC_STAGES - 1) ? 0.0f : t;        // (an analysis call: the back half did not run)
    }
    // Pipelined window control: the k_xf interval spans start-up + waits + the transform chunk launches.
    // Report the launches themselves as k_xf (what a kernel trace shows) and the rest as "wc_pipeline_exposed".
    if (n == ULCX_ENC_STAGES && n < maxStages) {
        const int IX_XF = 5;
        float exposed = 0.0f;
        if (e->nXf > 0) {
            float sum = 0.0f; bool ok = true;
            for (int j = 0; j < e->nXf; j++) { float t = 0; if (hipEventElapsedTime(&t, e->sync.xfTiming[2 * j], e->sync.xfTiming[2 * j + 1]) != hipSuccess) { ok = false; break; } sum += t; }
            if (ok) { exposed = ms[IX_XF] - sum; ms[IX_XF] = sum; }
        }
        ms[n++] = exposed;
    }
    return n;
}

extern "C" int ulcx_encoder_last_xf_launches(ulcx_encoder *e) { return (e && e->evRecorded) ? (e->nXf > 0 ? e->nXf : 1) : 0; }

// ---------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------
static void cleanup(ulcx_decoder *e) {
    if (!e) return;
    for (void *p : e->allocs) hipFree(p);
    if (e->tables) hipFree(e->tables);
    for (auto &l : e->low) if (l.tables) hipFree(l.tables);
    if (e->evOk) for (auto &v : e->ev) hipEventDestroy(v);
    block1_drop(e->b1);
    if (e->b1.stream) hipStreamDestroy(e->b1.stream);
    if (e->pinIn) hipHostFree(e->pinIn);
    if (e->pinPcm) hipHostFree(e->pinPcm);
    if (e->pinMeta) hipHostFree(e->pinMeta);
    delete e;
}
static int dec_reset_state(ulcx_decoder *e) {
    UlcxDecCtx &c = e->ctx;
    CKR(hipMemset(c.lap, 0, sizeof(float) * (size_t)e->B * e->C * (e->BS / 2)));     // ulcDecoder.c:56
    CKR(hipMemset(c.lastSub, 0, sizeof(int) * (size_t)e->B));                          // ulcDecoder.c:52
    CKR(hipMemset(c.dead, 0, sizeof(int) * (size_t)e->B));
    CKR(hipMemset(c.packOff, 0, sizeof(int) * (size_t)e->B));
    std::vector<uint32_t> seed((size_t)e->B, 1234567u);                                // ulcDecoder.c:76, one RNG per stream
    CKR(hipMemcpy(c.seed, seed.data(), sizeof(uint32_t) * seed.size(), hipMemcpyHostToDevice));
    e->b1Seed = 1234567u; e->b1SeedStale = false; e->inBlock1 = false;
    return ULCX_OK;
}

// One decode launch.  When the batch does not fill the machine in whole rounds of one workgroup per stream - 4096 streams on
// 1536 resident workgroups, or a few long streams - the synthesis takes an even cut of the (stream, block) pairs instead: a
// workgroup then runs one extra block (the one in front of its range, for the lapping state), so the cut must pay for that.
// The cut itself (host arithmetic, exported for the tests): workgroups of the synthesis for a call of nBlocks blocks of
// nStreams streams on a device that holds residentWG workgroups of the kernel; 0 = one workgroup per stream.  Cost in block
// times: ceil(streams / resident) rounds of nBlocks blocks against blocks-per-workgroup + 1 (the block in front of the range);
// the cut has to win by 1.5 x - an even cut of uneven streams ends with its slowest workgroup (measured on the bench batch).
extern "C" int ulcx_dec_split_plan(int nStreams, int nBlocks, int residentWG) {
    if (nStreams < 1 || nBlocks < 1 || residentWG < 1) return 0;
    const long long T = (long long)nStreams * nBlocks;
    long long per = (T + residentWG - 1) / residentWG; if (per < 8) per = 8;
    const long long grid = T / per;
    const long long costStream = (((long long)nStreams + residentWG - 1) / residentWG) * nBlocks;
    return (grid >= 1 && grid != nStreams && (per + 1) * 3 < costStream * 2) ? (int)grid : 0;
}
// Round 5: a batch runs in rounds of one workgroup per stream, and its last round is partly empty (4096 streams on 1536
// resident workgroups: 2.67 rounds).  The whole rounds stay as they are - the hardware hands a free slot the next stream,
// which evens out workgroups of different speed -; only the streams of the last round are cut, into pieces of
// ULCX_DSYN_TAIL_LEN blocks (a quarter of a longer call's) at the end of the grid, each of which runs one block in front of
// its range for the lapping state.  What the cut buys is a short end of the launch, what it costs is the extra block per
// piece.  Measured (profiles/NOTES_r05.md), synthesis of 32 blocks of 4096 / 2048 / 1024 / 5000 streams: 1.50 -> 1.44, 0.89
// -> 0.75, 0.485 -> 0.45, 1.81 -> 1.76 ms; ONE piece per slot (the even cut of the last round) 1.51, pieces of 4 blocks
// 1.47-1.49, every stream cut 1.53-1.59; calls of 16 blocks (two pieces per stream) -1 % / +1.5 %: not cut.
// Returns the number of pieces (0: no cut), *full = the leading workgroups that take one whole stream each.  The cut is
// taken when the last round is at most four fifths full and a stream has at least three pieces.
#define ULCX_DSYN_TAIL_LEN 8
extern "C" int ulcx_dec_tail_plan(int nStreams, int nBlocks, int residentWG, int *full) {
    if (full) *full = 0;
    if (nStreams < 1 || nBlocks < 3 * ULCX_DSYN_TAIL_LEN || residentWG < 1) return 0;
    const int rem = nStreams % residentWG;
    if (rem == 0 || (long long)rem * 5 > (long long)residentWG * 4) return 0;
    const int len = nBlocks / 4 > ULCX_DSYN_TAIL_LEN ? nBlocks / 4 : ULCX_DSYN_TAIL_LEN;     // (a long call: four pieces per stream)
    const long long n = (long long)rem * nBlocks / len;                                      // < 4 residentWG
    if (full) *full = nStreams - rem;
    return (int)n;
}
// Range calls (ulcx_decode_range_*).  Every workgroup that enters a stream runs the block in front of its range without output,
// a whole-stream workgroup too: a piece of the last round costs its blocks + 1 against nBlocks + 1 for a whole stream, so
// short calls are worth cutting as well, into shorter pieces (a quarter of the call, at least 2 blocks; three pieces per
// stream at least, i.e. calls of 6 blocks or more).  Calls of 24 blocks or more are cut as any other call is.  Only when
// there is a whole round in front of the last one.
extern "C" int ulcx_dec_range_tail_plan(int nStreams, int nBlocks, int residentWG, int *full) {
    if (nBlocks >= 3 * ULCX_DSYN_TAIL_LEN) return ulcx_dec_tail_plan(nStreams, nBlocks, residentWG, full);
    if (full) *full = 0;
    if (nStreams < 1 || nBlocks < 1 || residentWG < 1 || nStreams <= residentWG) return 0;
    const int len = nBlocks / 4 > 2 ? nBlocks / 4 : 2;
    if (nBlocks < 3 * len) return 0;
    const int rem = nStreams % residentWG;
    if (rem == 0 || (long long)rem * 5 > (long long)residentWG * 4) return 0;
    if (full) *full = nStreams - rem;
    return (int)((long long)rem * nBlocks / len);
}
extern "C" int ulcx_decoder_last_cut(ulcx_decoder *e, int *workgroups, int *wholeStreams, int *residentWG) {
    if (!e) return refuse("ulcx_decoder_last_cut", "no decoder");
    if (workgroups) *workgroups = e->lastGrid;
    if (wholeStreams) *wholeStreams = e->lastFull;
    if (residentWG) *residentWG = e->synSlots;
    return ULCX_OK;
}
// subsetSet != NULL: a subset call - c.B is the number of listed slots (what the cut is planned from) and c.lap .. c.dead are
// set 0 of the compact shadow state; a cut leaves its result in set 1 of THAT state, the object's own sets are not swapped,
// and *subsetSet receives the set that holds the result.
// call: what kind of call it is and that kind's arguments (NULL: a plain call).  A call on rows of its own - every kind behind ULCX_DEC_RANGE, with
// subsetSet: it runs on the shadow state as a subset call does - moves no stream's generator word, so the single-block path's host copy stays good.
static int dec_launch(ulcx_decoder *e, UlcxDecCtx &c, hipStream_t st, int *subsetSet = nullptr, const UlcxDecAux *call = nullptr) {
    UlcxDecAux a;
    if (call) a = *call;
    a.synGrid = 0; a.synFull = 0;
    const bool range = a.kind != ULCX_DEC_PLAIN, low = a.kind == ULCX_DEC_LOWRATE;
    if (!e->inBlock1 && a.kind <= ULCX_DEC_RANGE) e->b1SeedStale = true;   // (a batched / packed call on a one-stream decoder: see b1Seed)
    c.lapO = c.lap; c.lastSubO = c.lastSub; c.seedO = c.seed; c.deadO = c.dead;
    const int Kc = range ? c.K - 1 : c.K;                         // blocks of the call per stream (a range call's K counts the row of the block in front)
    // (a low-rate call: the cut is planned for the kernel of the reduced geometry - its residency, its scratch rows)
    const int synSlots = low ? e->low[a.low.lgD].synSlots : e->synSlots, scratchRows = low ? e->low[a.low.lgD].scratchRows : e->scratchRows;
    // (a spectra or distortion call has no synthesis to cut, and a part call's - k_dpart or k_dgen - runs one workgroup per row: the plain plan)
    if ((low || e->splitOK) && synSlots > 0 && ulcx_dec_has_synthesis(a.kind) && a.kind != ULCX_DEC_PART) {
        // A range call of more streams than the device holds at once: whole rounds, and the last one cut
        // (ulcx_dec_range_tail_plan) - an even cut of everything ends every workgroup inside a stream, and in a range call every
        // entry into a stream costs the block in front of the range (ULCX_RANGE_CUT=even: the even cut first, as for other calls)
        if (range && c.B > synSlots && e->tailCut && !e->rangeEvenFirst) {
            int full = 0;
            const int tail = ulcx_dec_range_tail_plan(c.B, Kc, synSlots, &full);
            if (tail > 0 && tail <= scratchRows) { a.synGrid = full + tail; a.synFull = full; }
        }
        if (!a.synGrid) a.synGrid = ulcx_dec_split_plan(c.B, Kc, synSlots);
        if (!a.synGrid) {
            int full = 0;
            const int tail = range ? ulcx_dec_range_tail_plan(c.B, Kc, synSlots, &full) : ulcx_dec_tail_plan(c.B, Kc, synSlots, &full);
            if (tail > 0 && tail <= scratchRows && e->tailCut) { a.synGrid = full + tail; a.synFull = full; }
        }
        if (a.synGrid) {
            if (getenv("ULCX_DEBUG_PRINT")) fprintf(stderr, "[ulcx] synthesis: %lld (stream, block) pairs over %d workgroups (%d of them one stream each; %d resident)\n", (long long)c.B * Kc, a.synGrid, a.synFull, synSlots);
            // (a range synthesis reads no state in front of the launch: a low-rate call leaves its rows' state in the set it names,
            //  so a file geometry without a second set - a non-fast one that feeds the stereo kernel - can be cut too)
            if (!low) {
                if (subsetSet) { c.lapO = e->subLap[1]; c.lastSubO = e->subLastSub[1]; c.seedO = e->subSeed[1]; c.deadO = e->subDead[1]; }
                else { c.lapO = e->lap2; c.lastSubO = e->lastSub2; c.seedO = e->seed2; c.deadO = e->dead2; }
            }
        }
    }
    e->lastGrid = a.synGrid; e->lastFull = a.synFull;
    const int rc = ulcx_dec_launch(c, st, e->timing ? e->ev : nullptr, a);
    if (subsetSet) *subsetSet = a.synGrid ? 1 : 0;
    else if (rc == ULCX_OK && a.synGrid) {
        std::swap(e->ctx.lap, e->lap2); std::swap(e->ctx.lastSub, e->lastSub2); std::swap(e->ctx.seed, e->seed2); std::swap(e->ctx.dead, e->dead2);
    }
    return rc;
}

// The synthesis kernel of a geometry (the object's, or a low-rate ratio's reduced one).  fastOK: stereo streams up to BlockSize 4096 take k_dsyn
// - both channels' FFT arrays in LDS, one wave per channel, the lapping state in global memory (ULCX_DEC_FAST=0: never) -, everything else the
// general kernel (k_dgen: one array).  twInLds: k_dsyn up to BlockSize 2048 keeps the FFT twiddles in LDS, above it they come from the tables.
static void dec_syn_geometry(int nChan, int BlockSize, int *fastOK, int *twInLds) {
    *fastOK = (nChan == 2 && BlockSize <= 4096) ? 1 : 0;
    if (const char *ev = getenv("ULCX_DEC_FAST")) *fastOK = *fastOK && (ev[0] != '0');
    *twInLds = (*fastOK && BlockSize <= 2048 && ULCX_DSYN_TWL) ? 1 : 0;
}
extern "C" int ulcx_decoder_create(ulcx_decoder **out, int device, int nStreams, int nChan, int BlockSize, int maxBlocksPerCall) {
    const char *who = "ulcx_decoder_create";
    if (!out) return refuse(who, "no place for the object");
    *out = nullptr;
    if (!validate(nChan, BlockSize) || nStreams < 1 || maxBlocksPerCall < 1) return refuse(who, "invalid decoder geometry");
    int rc = select_device(who, device);
    if (rc) return rc;
    ulcx_decoder *e = new ulcx_decoder();
    e->device = device; e->B = nStreams; e->C = nChan; e->BS = BlockSize; e->maxK = maxBlocksPerCall;
    UlcxDecCtx &c = e->ctx;
    c.B = nStreams; c.C = nChan; c.BS = BlockSize; c.lgBS = ilog2i(BlockSize); c.maxK = maxBlocksPerCall;
#ifdef ULCX_ABLATE
    if (const char *ev = getenv("ULCX_DBG_SKIP")) c.dbgSkip = atoi(ev);
#endif
    dec_syn_geometry(nChan, BlockSize, &c.fastOK, &c.twInLds);
    rc = ulcx_tables_build(&c.T, &e->tables, BlockSize, 44100, false);
    if (rc) { cleanup(e); return rc; }
    size_t B = nStreams, NB = B * maxBlocksPerCall;
    DA(c.lap, B * nChan * (BlockSize / 2), true);
    DA(c.lastSub, B, true);
    DA(c.seed, B, true);
    DA(c.dead, B, true);
    c.lapO = c.lap; c.lastSubO = c.lastSub; c.seedO = c.seed; c.deadO = c.dead; c.lapScratch = nullptr; c.k0 = 0; c.k1 = 0;
    if (c.fastOK) {                                                       // the kernel keeps the lapping state in global memory: any grid
        bool want = true;
        if (const char *ev = getenv("ULCX_DSYN_SPLIT")) want = ev[0] != '0';
        if (const char *ev = getenv("ULCX_DSYN_TAIL")) e->tailCut = ev[0] != '0';          // (A/B: the last round uncut)
        if (const char *ev = getenv("ULCX_RANGE_CUT")) e->rangeEvenFirst = !strcmp(ev, "even");   // (A/B: range calls planned as other calls are)
        e->synSlots = want ? ulcx_dec_syn_slots(c, ULCX_SYN_CUT) : 0;
        if (e->synSlots > 0) {
            DA(e->lap2, B * nChan * (BlockSize / 2), true);
            DA(e->lastSub2, B, true);
            DA(e->seed2, B, true);
            DA(e->dead2, B, true);
            e->scratchRows = 4 * e->synSlots;                              // (an even cut: <= synSlots workgroups; a cut of the last round: < synSlots streams in <= 4 pieces each)
            DA(c.lapScratch, (size_t)e->scratchRows * nChan * (BlockSize / 2), true);
            e->splitOK = true;
        }
    }
    DA(c.wcScan, NB, true);
    DA(c.draws, NB, true);
    DA(c.packOff, B, true);
    DA(c.blkOff, NB, true);
    DA(c.rInfo, B, true);
    DA(e->bitsScr, NB, true);
    DA(c.unitDraws, NB * nChan * 4, true);
    DA(c.unitTail, NB * nChan * 4, true);
    DA(c.unitRec, NB * nChan * 4, true);
    // what the scan leaves for the synthesis: at most one plain-run record per coefficient, one noise record per 16 (+ a tail per unit)
    c.precStride = nChan * BlockSize;
    c.nrecStride = nChan * BlockSize / 16 + nChan * 4;
    DA(c.prec, NB * (size_t)c.precStride, false);
    DA(c.nrec, NB * (size_t)c.nrecStride, false);
    c.tailStride = BlockSize / 32;
    DA(c.tailMag, NB * nChan * 4 * (size_t)c.tailStride, false);
    DA(c.scratch, B * 4 * (size_t)BlockSize, false);
    {
        std::vector<uint32_t> jt;
        build_rng_tables(jt);
        uint32_t *dj = nullptr;
        DA(dj, jt.size(), false);
        if (hipMemcpy(dj, jt.data(), sizeof(uint32_t) * jt.size(), hipMemcpyHostToDevice) != hipSuccess) { ulcx_set_error("hipMemcpy(rng tables)"); cleanup(e); return ULCX_ERR_HIP; }
        c.jumpT = dj;
        c.parT = dj + (size_t)8 * 16 * 4 * 256;
    }
    for (auto &v : e->ev) { if (hipEventCreate(&v) != hipSuccess) { ulcx_set_error("hipEventCreate failed"); cleanup(e); return ULCX_ERR_HIP; } }
    e->evOk = true;
    rc = dec_reset_state(e);
    if (rc) { cleanup(e); return rc; }
    *out = e;
    return ULCX_OK;
}
extern "C" void ulcx_decoder_destroy(ulcx_decoder *e) { if (e) { hipSetDevice(e->device); cleanup(e); } }
extern "C" int ulcx_decoder_reset(ulcx_decoder *e) { if (!e) return refuse("ulcx_decoder_reset", "no decoder"); CKR(hipSetDevice(e->device)); return dec_reset_state(e); }

// Device staging of the host-pointer entries, kept by the object: output samples and sizes of maxBlocksPerCall blocks of every
// stream; inBytes > 0: the input slots too, regrown for a larger slotBytes (a captured single-block sequence holds the old
// buffer's address: it is dropped with the buffer and captured again by the next single-block call)
static int dec_host_staging(ulcx_decoder *e, size_t inBytes) {
    const size_t nBlk = (size_t)e->B * e->maxK;
    int rc;
    if (inBytes && e->d_in_bytes < inBytes) {
        if (e->d_in) block1_drop(e->b1);
        e->d_in_bytes = 0;
        if ((rc = dregrow(e->allocs, &e->d_in, inBytes, true))) return rc;
        e->d_in_bytes = inBytes;
    }
    if (!e->d_pcm && (rc = dalloc(e->allocs, &e->d_pcm, nBlk * (size_t)e->C * e->BS, false))) return rc;
    if (!e->d_bits && (rc = dalloc(e->allocs, &e->d_bits, nBlk, false))) return rc;
    return ULCX_OK;
}

// ---- stream slots: the decoder's side (the object's CURRENT set of state arrays: e->ctx.lap .. - a cut synthesis swaps the sets)
static size_t dec_lap_bytes(const ulcx_decoder *e) { return sizeof(float) * (size_t)e->C * (e->BS / 2); }
extern "C" size_t ulcx_decoder_stream_state_bytes(const ulcx_decoder *e) { return e ? ULCX_STATE_HEADER + dec_lap_bytes(e) + 16 : 0; }
static size_t slot_state_bytes(const ulcx_decoder *e) { return ulcx_decoder_stream_state_bytes(e); }
// (a reset or a load changes the generator word behind the single-block path's host copy, as a batched decode call does: b1Seed)
static void slot_touch(ulcx_decoder *e) { if (!e->inBlock1) e->b1SeedStale = true; }
static UlcxSlotGeom slot_geom(const ulcx_decoder *e, bool /*record: the same layout*/) {
    UlcxSlotGeom g = {};
    g.B = e->B; g.rowVec = (int)(dec_lap_bytes(e) / 16); g.isEnc = 0; g.nSmall = 4; g.smallWords = 1; g.padWords = 1;
    g.header = make_uint4(ULCX_STATE_MAGIC_DEC, (unsigned)e->C, (unsigned)e->BS, 0u);
    return g;
}
static UlcxSlotRows dec_slot_rows(const ulcx_decoder *e, float *lap, int *lastSub, uint32_t *seed, int *dead, int *packOff) {
    UlcxSlotRows r = {};
    r.big = (uint8_t *)lap; r.bigStride = dec_lap_bytes(e);
    r.small[0] = (uint8_t *)lastSub; r.small[1] = (uint8_t *)seed; r.small[2] = (uint8_t *)dead; r.small[3] = (uint8_t *)packOff; r.smallStride = 4;
    return r;
}
static UlcxSlotRows slot_obj_rows(const ulcx_decoder *e) { return dec_slot_rows(e, e->ctx.lap, e->ctx.lastSub, e->ctx.seed, e->ctx.dead, e->ctx.packOff); }
static UlcxSlotRows dec_shadow_rows(const ulcx_decoder *e, int set) { return dec_slot_rows(e, e->subLap[set], e->subLastSub[set], e->subSeed[set], e->subDead[set], e->subPackOff); }
static UlcxSlotRows slot_record_rows(const ulcx_decoder *e, uint8_t *state) {
    UlcxSlotRows r = {};
    const size_t bytes = slot_state_bytes(e);
    r.hdr = state; r.hdrStride = bytes; r.big = state + ULCX_STATE_HEADER; r.bigStride = bytes;
    for (int a = 0; a < 4; a++) r.small[a] = state + ULCX_STATE_HEADER + dec_lap_bytes(e) + 4 * a;
    r.smallStride = bytes;
    return r;
}
static int dec_shadow(ulcx_decoder *e) {
    int rc;
    for (int set = 0; set < (e->splitOK ? 2 : 1); set++) {
        if (!e->subLap[set] && (rc = dalloc(e->allocs, &e->subLap[set], (size_t)e->B * e->C * (e->BS / 2), false))) return rc;
        if (!e->subLastSub[set] && (rc = dalloc(e->allocs, &e->subLastSub[set], (size_t)e->B, false))) return rc;
        if (!e->subSeed[set] && (rc = dalloc(e->allocs, &e->subSeed[set], (size_t)e->B, false))) return rc;
        if (!e->subDead[set] && (rc = dalloc(e->allocs, &e->subDead[set], (size_t)e->B, false))) return rc;
    }
    if (!e->subPackOff && (rc = dalloc(e->allocs, &e->subPackOff, (size_t)e->B, false))) return rc;
    if (!e->sampRows && (rc = dalloc(e->allocs, &e->sampRows, 4 * (size_t)e->B, false))) return rc;
    return ULCX_OK;
}

// ---- the decoder's call families, as the encoder's: a public entry names itself to the body of its family, which makes every
// check before any device work.
//   decode_dev_any     slots in, whole object or subset       decode_packed_any   the next blocks of packed payloads
//   decode_range_any   any block range of packed payloads     index_packed_any    the block index
// The host-pointer forms check, stage (dec_host_staging for what the object keeps, a DevTmp for what lives for the call), run the
// body on the null stream and fetch the results with dec_results_down.
// the arguments every decode entry has: in = slots or payloads, pcm = the one sample pointer the entry takes; device or host
// front = 1: a range call (the block in front of a range takes one row of the per-block scratch: nBlocks <= maxBlocksPerCall - 1)
static int dec_args_bad(const char *who, const ulcx_decoder *e, const void *in, const void *pcm, const void *bits, int nBlocks, int front) {
    if (e && in && pcm && bits && nBlocks >= 1 && nBlocks <= e->maxK - front) return 0;
    refuse(who, front ? "bad argument (nBlocks is 1 .. maxBlocksPerCall - 1)" : "bad argument");
    return 1;
}
// subset: the entry takes a slot list, as the encoder's (encode_dev_any): gather, the plain launch on the compact state, scatter
static int decode_dev_any(const char *who, ulcx_decoder *e, const uint8_t *d_in, int slotBytes, int nBlocks, float *d_pcm, int16_t *d_pcm16, int32_t *d_bits, void *hipStream,
                          bool subset = false, const int32_t *d_slots = nullptr, int n = 0) {
    if (dec_args_bad(who, e, d_in, d_pcm ? (const void *)d_pcm : d_pcm16, d_bits, nBlocks, 0)) return ULCX_ERR_ARG;
    if (slotBytes < 1) return refuse(who, "bad argument");
    if (subset && slots_list_bad(who, d_slots, n, e->B)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16) ||
        misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.K = nBlocks; c.slot = slotBytes; c.in = d_in; c.pcm = d_pcm; c.pcm16 = d_pcm16; c.bits = d_bits;
    c.inBytes = (long long)e->B * nBlocks * slotBytes;
    if (subset) {
        int rc0 = dec_shadow(e);
        if (!rc0) rc0 = ulcx_slots_gather(slot_obj_rows(e), dec_shadow_rows(e, 0), d_slots, n, slot_geom(e, false), (hipStream_t)hipStream);
        if (rc0) return rc0;
        c.B = n; c.inBytes = (long long)n * nBlocks * slotBytes;
        c.lap = e->subLap[0]; c.lastSub = e->subLastSub[0]; c.seed = e->subSeed[0]; c.dead = e->subDead[0]; c.packOff = e->subPackOff;
    }
    int set = 0;
    int rc = dec_launch(e, c, (hipStream_t)hipStream, subset ? &set : nullptr);
    if (subset && rc == ULCX_OK) rc = ulcx_slots_scatter(slot_obj_rows(e), dec_shadow_rows(e, set), d_slots, n, slot_geom(e, false), (hipStream_t)hipStream);
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    return rc;
}
extern "C" int ulcx_decode_dev(ulcx_decoder *e, const uint8_t *d_in, int slotBytes, int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_dev_any("ulcx_decode_dev", e, d_in, slotBytes, nBlocks, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_dev_pcm16(ulcx_decoder *e, const uint8_t *d_in, int slotBytes, int nBlocks, int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return decode_dev_any("ulcx_decode_dev_pcm16", e, d_in, slotBytes, nBlocks, nullptr, d_pcm16, d_bits, hipStream);
}
extern "C" int ulcx_decode_dev_subset(ulcx_decoder *e, const int32_t *d_slots, int n, const uint8_t *d_in, int slotBytes, int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_dev_any("ulcx_decode_dev_subset", e, d_in, slotBytes, nBlocks, d_pcm, nullptr, d_bits, hipStream, true, d_slots, n);
}
extern "C" int ulcx_decode_dev_pcm16_subset(ulcx_decoder *e, const int32_t *d_slots, int n, const uint8_t *d_in, int slotBytes, int nBlocks, int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return decode_dev_any("ulcx_decode_dev_pcm16_subset", e, d_in, slotBytes, nBlocks, nullptr, d_pcm16, d_bits, hipStream, true, d_slots, n);
}
// waits for the device, then copies the samples and sizes of NB blocks down
static int dec_results_down(ulcx_decoder *e, const float *d_pcm, const int32_t *d_bits, size_t NB, float *h_pcm, int32_t *h_bits) {
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_pcm, d_pcm, sizeof(float) * NB * (size_t)e->C * e->BS, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_bits, d_bits, sizeof(int32_t) * NB, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
static int decode_host_any(const char *who, ulcx_decoder *e, const uint8_t *h_in, int slotBytes, int nBlocks, float *h_pcm, int32_t *h_bits,
                           bool subset = false, const int32_t *h_slots = nullptr, int n = 0) {
    if (dec_args_bad(who, e, h_in, h_pcm, h_bits, nBlocks, 0)) return ULCX_ERR_ARG;
    if (slotBytes < 1) return refuse(who, "bad argument");
    if (subset && slots_host_bad(who, h_slots, n, e->B)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t NBmax = (size_t)e->B * e->maxK, NB = (subset ? (size_t)n : (size_t)e->B) * nBlocks;
    int rc = dec_host_staging(e, NBmax * (size_t)slotBytes + 16);
    if (!rc && subset) rc = slots_list_up(e, h_slots, n);
    if (rc) return rc;
    CKR(hipMemcpy(e->d_in, h_in, NB * slotBytes, hipMemcpyHostToDevice));
    rc = decode_dev_any(who, e, e->d_in, slotBytes, nBlocks, e->d_pcm, nullptr, e->d_bits, nullptr, subset, e->subSlots, n);
    return rc ? rc : dec_results_down(e, e->d_pcm, e->d_bits, NB, h_pcm, h_bits);
}
extern "C" int ulcx_decode_host(ulcx_decoder *e, const uint8_t *h_in, int slotBytes, int nBlocks, float *h_pcm, int32_t *h_bits) {
    return decode_host_any("ulcx_decode_host", e, h_in, slotBytes, nBlocks, h_pcm, h_bits);
}
extern "C" int ulcx_decode_host_subset(ulcx_decoder *e, const int32_t *h_slots, int n, const uint8_t *h_in, int slotBytes, int nBlocks, float *h_pcm, int32_t *h_bits) {
    return decode_host_any("ulcx_decode_host_subset", e, h_in, slotBytes, nBlocks, h_pcm, h_bits, true, h_slots, n);
}

// One block of one stream per call, as ulcx_encode_block1.
// rngState: the noise generator's state (ulcDecoder.c:75-81) before the block in, after it out.  The reference keeps it in a
// function-static word, i.e. ONE state per process that every decoder object draws from; a caller that wants that behaviour
// (the drop-in of section 1 does) owns the word and hands it through here.  NULL: the state stays with this decoder object.
static int decode_block1_any(const char *who, ulcx_decoder *e, const uint8_t *h_in, int nBytes, float *h_pcm, int32_t *bits, int32_t *lastSubBlockSize, uint32_t *rngState) {
    if (!e || !h_in || !h_pcm || nBytes < 1 || e->B != 1 || e->maxK != 1) return refuse(who, "needs a decoder of one stream, one block per call");
    CKR(hipSetDevice(e->device));
    const size_t cb = (size_t)e->C * e->BS;
    const int slot = 2 * e->C * e->BS + 16;                       // the largest block
    if (nBytes > slot) nBytes = slot;
    if (!e->b1Init) {
        int rc;
        if ((rc = dec_host_staging(e, (size_t)slot + 16))) return rc;                // (one stream, one block per call)
        if (!e->b1.stream) CKR(hipStreamCreateWithFlags(&e->b1.stream, hipStreamNonBlocking));
        if (!e->pinIn) CKR(hipHostMalloc((void **)&e->pinIn, (size_t)slot, hipHostMallocDefault));
        if (!e->pinPcm) CKR(hipHostMalloc((void **)&e->pinPcm, sizeof(float) * cb, hipHostMallocDefault));
        if (!e->pinMeta) CKR(hipHostMalloc((void **)&e->pinMeta, 4 * sizeof(int32_t), hipHostMallocDefault));
        e->b1Init = true; e->b1Slot = slot;
        e->timing = false;
    }
    auto enqueue = [&]() -> int {
        CKR(hipMemcpyAsync(e->d_in, e->pinIn, (size_t)slot, hipMemcpyHostToDevice, e->b1.stream));
        CKR(hipMemcpyAsync(e->ctx.seed, &e->pinMeta[2], sizeof(uint32_t), hipMemcpyHostToDevice, e->b1.stream));
        int rc = decode_dev_any(who, e, e->d_in, slot, 1, e->d_pcm, nullptr, e->d_bits, e->b1.stream);
        if (rc) return rc;
        CKR(hipMemcpyAsync(&e->pinMeta[3], e->ctx.seed, sizeof(uint32_t), hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(e->pinPcm, e->d_pcm, sizeof(float) * cb, hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta[0], e->d_bits, sizeof(int32_t), hipMemcpyDeviceToHost, e->b1.stream));
        CKR(hipMemcpyAsync(&e->pinMeta[1], e->ctx.lastSub, sizeof(int32_t), hipMemcpyDeviceToHost, e->b1.stream));
        return ULCX_OK;
    };
    memcpy(e->pinIn, h_in, (size_t)nBytes);
    memset(e->pinIn + nBytes, 0, (size_t)(slot - nBytes));         // (only the block's own bytes are the caller's: the rest of the slot reads as zero)
    if (!rngState && e->b1SeedStale) {                            // mixed use: ulcx_decode_dev / _host / _packed ran on this object since
        CKR(hipDeviceSynchronize());
        CKR(hipMemcpy(&e->b1Seed, e->ctx.seed, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    e->b1SeedStale = false;
    e->pinMeta[2] = (int32_t)(rngState ? *rngState : e->b1Seed);
    struct InB1 { ulcx_decoder *d; InB1(ulcx_decoder *x) : d(x) { d->inBlock1 = true; } ~InB1() { d->inBlock1 = false; } } inB1(e);
    { int rc = block1_run(e->b1, enqueue); if (rc) return rc; }
    memcpy(h_pcm, e->pinPcm, sizeof(float) * cb);
    if (bits) *bits = e->pinMeta[0];
    if (lastSubBlockSize) *lastSubBlockSize = e->pinMeta[1];
    e->b1Seed = (uint32_t)e->pinMeta[3];
    if (rngState) *rngState = e->b1Seed;
    return ULCX_OK;
}
extern "C" int ulcx_decode_block1(ulcx_decoder *e, const uint8_t *h_in, int nBytes, float *h_pcm, int32_t *bits, int32_t *lastSubBlockSize) {
    return decode_block1_any("ulcx_decode_block1", e, h_in, nBytes, h_pcm, bits, lastSubBlockSize, nullptr);
}
extern "C" int ulcx_decode_block1_rng(ulcx_decoder *e, const uint8_t *h_in, int nBytes, float *h_pcm, int32_t *bits, int32_t *lastSubBlockSize, uint32_t *rngState) {
    return decode_block1_any("ulcx_decode_block1_rng", e, h_in, nBytes, h_pcm, bits, lastSubBlockSize, rngState);
}

// ---------------------------------------------------------------------------
// .ulc container + packed streams (tools/ulc_Helper.h:10-20, ulcEncodeTool.c:92-100,160-195, ulcDecodeTool.c:73-80,123-166)
// ---------------------------------------------------------------------------
static void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
static void put32(uint8_t *p, uint32_t v) { put16(p, v); put16(p + 2, v >> 16); }
static uint32_t get16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t get32(const uint8_t *p) { return get16(p) | (get16(p + 2) << 16); }
extern "C" void ulcx_ulc_header_pack(uint8_t dst[24], const ulcx_file_header *h) {
    put32(dst + 0x00, h->Magic); put16(dst + 0x04, h->BlockSize); put16(dst + 0x06, h->MaxBlockSize);
    put32(dst + 0x08, h->nBlocks); put32(dst + 0x0C, h->RateHz); put16(dst + 0x10, h->nChan);
    put16(dst + 0x12, h->RateKbps); put32(dst + 0x14, h->StreamOffs);
}
extern "C" int ulcx_ulc_header_parse(ulcx_file_header *h, const uint8_t *src, size_t len) {
    if (!h || !src || len < 24) return refuse("ulcx_ulc_header_parse", "need 24 bytes");
    h->Magic = get32(src); h->BlockSize = (uint16_t)get16(src + 4); h->MaxBlockSize = (uint16_t)get16(src + 6);
    h->nBlocks = get32(src + 8); h->RateHz = get32(src + 12); h->nChan = (uint16_t)get16(src + 16);
    h->RateKbps = (uint16_t)get16(src + 18); h->StreamOffs = get32(src + 20);
    if (h->Magic != ULCX_ULC_MAGIC) return refuse("ulcx_ulc_header_parse", "not a ULC2 container");   /* ulcDecodeTool.c:77-80 */
    return ULCX_OK;
}
// `.ulx` sidecar (include/ulc_amd.h): 16 bytes in front of a file's index entries
extern "C" void ulcx_ulx_header_pack(uint8_t dst[16], const ulcx_index_file_header *h) {
    put32(dst + 0x00, h->Magic); put16(dst + 0x04, h->BlockSize); put16(dst + 0x06, h->nChan);
    put32(dst + 0x08, h->nBlocks); put32(dst + 0x0C, h->PayloadBytes);
}
extern "C" int ulcx_ulx_header_parse(ulcx_index_file_header *h, const uint8_t *src, size_t len) {
    if (!h || !src || len < ULCX_ULX_HEADER_BYTES) return refuse("ulcx_ulx_header_parse", "need 16 bytes");
    h->Magic = get32(src); h->BlockSize = (uint16_t)get16(src + 4); h->nChan = (uint16_t)get16(src + 6);
    h->nBlocks = get32(src + 8); h->PayloadBytes = get32(src + 12);
    if (h->Magic != ULCX_ULX_MAGIC) return refuse("ulcx_ulx_header_parse", "not a ULX1 block index");
    return ULCX_OK;
}
extern "C" int ulcx_ulc_rate_kbps(uint64_t totalBytes, uint32_t RateHz, uint32_t BlockSize, uint32_t nBlocks) {
    double avg = (double)totalBytes * 8.0 * RateHz / 1000.0 / ((double)BlockSize * nBlocks);          /* ulcEncodeTool.c:173,190 */
    return (int)lrint(avg);
}
extern "C" int ulcx_pack_streams_dev(int device, int nStreams, int nBlocks, int slotBytes, const uint8_t *d_slots, const int32_t *d_bits,
                                     uint8_t *d_payload, long long payloadStride, int32_t *d_payloadBytes, int32_t *d_maxBlock, void *hipStream) {
    if (nStreams < 1 || nBlocks < 1 || slotBytes < 1 || !d_slots || !d_bits || !d_payload || !d_payloadBytes || payloadStride < 1) { ulcx_set_error("ulcx_pack_streams_dev: bad argument"); return ULCX_ERR_ARG; }
    if (misaligned("ulcx_pack_streams_dev", "d_bits", d_bits, ULCX_ALIGN_WORD) || misaligned("ulcx_pack_streams_dev", "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) ||
        misaligned("ulcx_pack_streams_dev", "d_maxBlock", d_maxBlock, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    int rc = select_device("ulcx_pack_streams_dev", device);
    if (rc) return rc;
    return ulcx_pack_launch(nStreams, nBlocks, slotBytes, d_slots, d_bits, d_payload, payloadStride, d_payloadBytes, d_maxBlock, (hipStream_t)hipStream);
}
static int decode_packed_any(const char *who, ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                             int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream) {
    if (dec_args_bad(who, e, d_payload, d_pcm, d_bits, nBlocks, 0)) return ULCX_ERR_ARG;
    if (!d_payloadBytes || payloadStride < 1) return refuse(who, "bad argument");
    if (misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) ||
        misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.K = nBlocks; c.slot = 0; c.in = d_payload; c.pcm = d_pcm; c.pcm16 = nullptr; c.bits = d_bits;
    c.packed = 1; c.payStride = payloadStride; c.payBytes = d_payloadBytes;
    c.inBytes = (long long)e->B * payloadStride;
    int rc = dec_launch(e, c, (hipStream_t)hipStream);
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    return rc;
}
extern "C" int ulcx_decode_packed_dev(ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                      int nBlocks, float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_packed_any("ulcx_decode_packed_dev", e, d_payload, payloadStride, d_payloadBytes, nBlocks, d_pcm, d_bits, hipStream);
}
// the payloads and their sizes of a host-pointer call, into buffers of the call's own (zeroed: `pad` bytes behind the last payload)
static int payload_up(ulcx_decoder *e, DevTmp &t, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes, size_t pad, uint8_t **dp, int32_t **dn) {
    const size_t bytes = (size_t)e->B * (size_t)payloadStride;
    CKR(t.get(dp, bytes + pad)); CKR(t.get(dn, sizeof(int32_t) * e->B));
    if (pad) CKR(hipMemset(*dp, 0, bytes + pad));
    CKR(hipMemcpy(*dp, h_payload, bytes, hipMemcpyHostToDevice));
    CKR(hipMemcpy(*dn, h_payloadBytes, sizeof(int32_t) * e->B, hipMemcpyHostToDevice));
    return ULCX_OK;
}
extern "C" int ulcx_decode_packed_host(ulcx_decoder *e, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                       int nBlocks, float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_packed_host";
    if (dec_args_bad(who, e, h_payload, h_pcm, h_bits, nBlocks, 0)) return ULCX_ERR_ARG;
    if (!h_payloadBytes || payloadStride < 1) return refuse(who, "bad argument");
    CKR(hipSetDevice(e->device));
    const size_t NB = (size_t)e->B * nBlocks;
    DevTmp t; uint8_t *dp = nullptr; int32_t *dn = nullptr, *dbits = nullptr; float *dpcm = nullptr;
    int rc = payload_up(e, t, h_payload, payloadStride, h_payloadBytes, 16, &dp, &dn);
    if (rc) return rc;
    CKR(t.get(&dpcm, sizeof(float) * NB * (size_t)e->C * e->BS)); CKR(t.get(&dbits, sizeof(int32_t) * NB));
    rc = decode_packed_any(who, e, dp, payloadStride, dn, nBlocks, dpcm, dbits, nullptr);
    return rc ? rc : dec_results_down(e, dpcm, dbits, NB, h_pcm, h_bits);
}

// Whole files: the payloads go to the device once, every later call decodes the next nBlocks of every stream from there
// (ulcx_decode_packed_host re-uploads everything per call: fine for one call, quadratic over a long file).
// A failed upload leaves the object without a payload (and without the index of the one before: it belongs to its payload).
extern "C" int ulcx_decoder_upload_payload(ulcx_decoder *e, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes) {
    if (!e || !h_payload || !h_payloadBytes || payloadStride < 1) return refuse("ulcx_decoder_upload_payload", "bad argument");
    CKR(hipSetDevice(e->device));
    dfree(e->allocs, &e->d_index); e->idxStride = 0;
    const size_t bytes = (size_t)e->B * (size_t)payloadStride;
    int rc = dregrow(e->allocs, &e->d_pay, bytes + 16, true);
    if (!rc) rc = dregrow(e->allocs, &e->d_payBytes, (size_t)e->B, false);
    if (!rc && (hipMemcpy(e->d_pay, h_payload, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(e->d_payBytes, h_payloadBytes, sizeof(int32_t) * e->B, hipMemcpyHostToDevice) != hipSuccess)) {
        ulcx_set_error("ulcx_decoder_upload_payload: hipMemcpy: %s", hipGetErrorString(hipGetLastError()));
        rc = ULCX_ERR_HIP;
    }
    if (rc) { dfree(e->allocs, &e->d_pay); return rc; }
    e->payStride = payloadStride;
    return ulcx_decoder_reset(e);
}
extern "C" int ulcx_decode_resident_host(ulcx_decoder *e, int nBlocks, float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_resident_host";
    if (!e || !h_pcm || !h_bits || nBlocks < 1 || nBlocks > e->maxK) return refuse(who, "bad argument");
    if (!e->d_pay) return refuse(who, "no payload uploaded");
    CKR(hipSetDevice(e->device));
    int rc = dec_host_staging(e, 0);
    if (!rc) rc = decode_packed_any(who, e, e->d_pay, e->payStride, e->d_payBytes, nBlocks, e->d_pcm, e->d_bits, nullptr);
    return rc ? rc : dec_results_down(e, e->d_pcm, e->d_bits, (size_t)e->B * nBlocks, h_pcm, h_bits);
}

// ---------------------------------------------------------------------------
// Block index and range decode (include/ulc_amd.h section 3)
// ---------------------------------------------------------------------------
static int index_packed_any(const char *who, ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                            int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream) {
    if (!e || !d_payload || !d_payloadBytes || !d_index || !d_nBlocks || payloadStride < 1 || maxBlocks < 1) return refuse(who, "bad argument");
    if (misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_nBlocks", d_nBlocks, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.in = d_payload; c.packed = 1; c.payStride = payloadStride; c.payBytes = d_payloadBytes;
    c.inBytes = (long long)e->B * payloadStride;
    return ulcx_index_launch(c, maxBlocks, d_index, d_nBlocks, (hipStream_t)hipStream);
}
extern "C" int ulcx_index_packed_dev(ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                     int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream) {
    return index_packed_any("ulcx_index_packed_dev", e, d_payload, payloadStride, d_payloadBytes, maxBlocks, d_index, d_nBlocks, hipStream);
}
extern "C" int ulcx_index_packed_host(ulcx_decoder *e, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                      int maxBlocks, ulcx_index_entry *h_index, int32_t *h_nBlocks) {
    const char *who = "ulcx_index_packed_host";
    if (!e || !h_payload || !h_payloadBytes || !h_index || !h_nBlocks || payloadStride < 1 || maxBlocks < 1) return refuse(who, "bad argument");
    CKR(hipSetDevice(e->device));
    DevTmp t; uint8_t *dp = nullptr; int32_t *dn = nullptr, *dcnt = nullptr; ulcx_index_entry *di = nullptr;
    const size_t nEnt = (size_t)e->B * ((size_t)maxBlocks + 1);
    int rc = payload_up(e, t, h_payload, payloadStride, h_payloadBytes, 0, &dp, &dn);
    if (rc) return rc;
    CKR(t.get(&dcnt, sizeof(int32_t) * e->B)); CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt));
    if ((rc = index_packed_any(who, e, dp, payloadStride, dn, maxBlocks, di, dcnt, nullptr))) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_index, di, sizeof(ulcx_index_entry) * nEnt, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_nBlocks, dcnt, sizeof(int32_t) * e->B, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
static int decode_range_any(const char *who, ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                            const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks, const int32_t *d_first, int nBlocks,
                            float *d_pcm, int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    if (dec_args_bad(who, e, d_payload, d_pcm ? (const void *)d_pcm : d_pcm16, d_bits, nBlocks, 1)) return ULCX_ERR_ARG;
    if (!d_payloadBytes || !d_index || !d_indexBlocks || !d_first || payloadStride < 1 || indexStride < 1) return refuse(who, "bad argument (nBlocks is 1 .. maxBlocksPerCall - 1)");
    if (misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_indexBlocks", d_indexBlocks, ULCX_ALIGN_WORD) || misaligned(who, "d_first", d_first, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16) ||
        misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.K = nBlocks + 1; c.slot = 0; c.in = d_payload; c.pcm = d_pcm; c.pcm16 = d_pcm16;
    c.bits = e->bitsScr; c.bitsOut = d_bits;
    c.packed = 1; c.payStride = payloadStride; c.payBytes = d_payloadBytes;
    c.inBytes = (long long)e->B * payloadStride;
    c.range = 1; c.rIndex = d_index; c.rIndexStride = indexStride; c.rIndexBlocks = d_indexBlocks; c.rFirst = d_first;
    UlcxDecAux call = {}; call.kind = ULCX_DEC_RANGE;
    int rc = dec_launch(e, c, (hipStream_t)hipStream, nullptr, &call);
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    return rc;
}
extern "C" int ulcx_decode_range_dev(ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                     const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks, const int32_t *d_first, int nBlocks,
                                     float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_range_any("ulcx_decode_range_dev", e, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks, d_first, nBlocks, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_range_dev_pcm16(ulcx_decoder *e, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                           const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks, const int32_t *d_first, int nBlocks,
                                           int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return decode_range_any("ulcx_decode_range_dev_pcm16", e, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks, d_first, nBlocks, nullptr, d_pcm16, d_bits, hipStream);
}
// the range starts of a host form: none negative (what the device forms cannot refuse)
static int range_first_bad(const char *who, const ulcx_decoder *e, const int32_t *h_first) {
    for (int s = 0; s < e->B; s++) if (h_first[s] < 0) { refuse(who, "stream %d starts at block %d", s, (int)h_first[s]); return 1; }
    return 0;
}
extern "C" int ulcx_decode_range_host(ulcx_decoder *e, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                      const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks, const int32_t *h_first, int nBlocks,
                                      float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_range_host";
    if (dec_args_bad(who, e, h_payload, h_pcm, h_bits, nBlocks, 1)) return ULCX_ERR_ARG;
    if (!h_payloadBytes || !h_index || !h_indexBlocks || !h_first || payloadStride < 1 || indexStride < 1) return refuse(who, "bad argument (nBlocks is 1 .. maxBlocksPerCall - 1)");
    if (range_first_bad(who, e, h_first)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t NB = (size_t)e->B * nBlocks, nEnt = (size_t)e->B * (size_t)indexStride;
    DevTmp t; uint8_t *dp = nullptr; int32_t *dn = nullptr, *dcnt = nullptr, *df = nullptr, *dbits = nullptr; ulcx_index_entry *di = nullptr; float *dpcm = nullptr;
    int rc = payload_up(e, t, h_payload, payloadStride, h_payloadBytes, 0, &dp, &dn);
    if (rc) return rc;
    CKR(t.get(&dcnt, sizeof(int32_t) * e->B)); CKR(t.get(&df, sizeof(int32_t) * e->B));
    CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt)); CKR(t.get(&dpcm, sizeof(float) * NB * (size_t)e->C * e->BS)); CKR(t.get(&dbits, sizeof(int32_t) * NB));
    CKR(hipMemcpy(dcnt, h_indexBlocks, sizeof(int32_t) * e->B, hipMemcpyHostToDevice));
    CKR(hipMemcpy(df, h_first, sizeof(int32_t) * e->B, hipMemcpyHostToDevice));
    CKR(hipMemcpy(di, h_index, sizeof(ulcx_index_entry) * nEnt, hipMemcpyHostToDevice));
    rc = decode_range_any(who, e, dp, payloadStride, dn, di, indexStride, dcnt, df, nBlocks, dpcm, nullptr, dbits, nullptr);
    return rc ? rc : dec_results_down(e, dpcm, dbits, NB, h_pcm, h_bits);
}
extern "C" int ulcx_decoder_index_resident(ulcx_decoder *e, int maxBlocks, int32_t *h_nBlocks) {
    const char *who = "ulcx_decoder_index_resident";
    if (!e || maxBlocks < 1) return refuse(who, "bad argument");
    if (!e->d_pay) return refuse(who, "no payload uploaded");
    CKR(hipSetDevice(e->device));
    e->idxStride = 0;
    int rc = dregrow(e->allocs, &e->d_index, (size_t)e->B * ((size_t)maxBlocks + 1), false);
    if (!rc && !e->d_idxBlocks) rc = dalloc(e->allocs, &e->d_idxBlocks, (size_t)e->B, false);
    if (!rc) rc = index_packed_any(who, e, e->d_pay, e->payStride, e->d_payBytes, maxBlocks, e->d_index, e->d_idxBlocks, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    e->idxStride = maxBlocks + 1;
    if (h_nBlocks) CKR(hipMemcpy(h_nBlocks, e->d_idxBlocks, sizeof(int32_t) * e->B, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
extern "C" int ulcx_decode_resident_range_host(ulcx_decoder *e, const int32_t *h_first, int nBlocks, float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_resident_range_host";
    if (dec_args_bad(who, e, h_first, h_pcm, h_bits, nBlocks, 1)) return ULCX_ERR_ARG;
    if (!e->d_pay || !e->idxStride) return refuse(who, "no payload uploaded, or not indexed (ulcx_decoder_index_resident)");
    if (range_first_bad(who, e, h_first)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    int rc = dec_host_staging(e, 0);
    if (!rc && !e->d_first) rc = dalloc(e->allocs, &e->d_first, (size_t)e->B, true);
    if (rc) return rc;
    CKR(hipMemcpy(e->d_first, h_first, sizeof(int32_t) * e->B, hipMemcpyHostToDevice));
    rc = decode_range_any(who, e, e->d_pay, e->payStride, e->d_payBytes, e->d_index, e->idxStride, e->d_idxBlocks, e->d_first, nBlocks, e->d_pcm, nullptr, e->d_bits, nullptr);
    return rc ? rc : dec_results_down(e, e->d_pcm, e->d_bits, (size_t)e->B * nBlocks, h_pcm, h_bits);
}

// ---- the corpus of a call (UlcxCorpus, ulcx_internal.h): every entry of the crop, sample-crop, spectra and splice families builds
// it once from its public arguments (ulcx_corpus_strided / ulcx_corpus_ragged), and from there on it is one argument.  What the
// families check of it, in the pieces their orders of refusal need: its pointers, the scalars of its layout, its alignments.
static bool corpus_null(const UlcxCorpus &g) { return !g.pay || !g.index || !g.indexBlocks || (g.ragged ? (!g.payOffs || !g.idxOffs) : !g.payBytes); }
static int corpus_layout_bad(const char *who, const UlcxCorpus &g) {
    if (g.ragged ? (g.payTotal >= 0 && g.idxTotal >= 0) : (g.payStride >= 1 && g.indexStride >= 1)) return 0;
    if (g.ragged) refuse(who, "bad argument (payloadTotal %lld, indexTotal %lld)", g.payTotal, g.idxTotal);
    else refuse(who, "bad argument (payloadStride %lld, indexStride %d)", g.payStride, g.indexStride);
    return 1;
}
static int corpus_misaligned(const char *who, const UlcxCorpus &g) {
    return misaligned(who, "d_payloadOffs", g.payOffs, ULCX_ALIGN_OFFS) || misaligned(who, "d_indexOffs", g.idxOffs, ULCX_ALIGN_OFFS) ||
           misaligned(who, "d_payloadBytes", g.payBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_index", g.index, ULCX_ALIGN_WORD) ||
           misaligned(who, "d_indexBlocks", g.indexBlocks, ULCX_ALIGN_WORD);
}
// What only a host form can refuse of a corpus, and its way to the device.
// the two tables of a ragged corpus: offsets that are negative, fall or leave their buffer, a file of 2^31 bytes or more
static int ragged_tables_bad(const char *who, const UlcxCorpus &g) {
    for (int f = 0; f < g.nFiles; f++) {
        const long long p0 = g.payOffs[f], p1 = g.payOffs[f + 1], i0 = g.idxOffs[f], i1 = g.idxOffs[f + 1];
        if (p0 < 0 || p1 < p0 || p1 > g.payTotal || p1 - p0 >= 0x80000000LL) { refuse(who, "file %d is bytes %lld .. %lld of a payload buffer of %lld", f, p0, p1, g.payTotal); return 1; }
        if (i0 < 0 || i1 < i0 || i1 > g.idxTotal) { refuse(who, "file %d has index entries %lld .. %lld of %lld", f, i0, i1, g.idxTotal); return 1; }
    }
    return 0;
}
// row i names file f: refused outside the corpus, else *nI = the file's blocks as the walk reads the count (ulcx_row_blocks)
static int host_row_file(const char *who, const UlcxCorpus &g, int i, int f, long long *nI) {
    if (f < 0 || f >= g.nFiles) { refuse(who, "row %d names file %d of %d", i, f, g.nFiles); return 1; }
    *nI = ulcx_row_blocks(g.indexBlocks[f], g.ragged ? g.idxOffs[f + 1] - g.idxOffs[f] : g.indexStride);
    return 0;
}
// nRows payloads and their sizes of a host-pointer call, into buffers of the call's own (payload_up with a row count of its own)
static int payload_rows_up(DevTmp &t, int nRows, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes, uint8_t **dp, int32_t **dn) {
    const size_t bytes = (size_t)nRows * (size_t)payloadStride;
    CKR(t.get(dp, bytes)); CKR(t.get(dn, sizeof(int32_t) * (size_t)nRows));
    CKR(hipMemcpy(*dp, h_payload, bytes, hipMemcpyHostToDevice));
    CKR(hipMemcpy(*dn, h_payloadBytes, sizeof(int32_t) * (size_t)nRows, hipMemcpyHostToDevice));
    return ULCX_OK;
}
// the same for a ragged corpus: its buffer and its two tables (*d: h with these three on the device)
static int ragged_up(DevTmp &t, const UlcxCorpus &h, UlcxCorpus *d) {
    const size_t tb = sizeof(int64_t) * ((size_t)h.nFiles + 1);
    uint8_t *dp = nullptr; int64_t *po = nullptr, *io = nullptr;
    CKR(t.get(&dp, (size_t)h.payTotal)); CKR(t.get(&po, tb)); CKR(t.get(&io, tb));
    if (h.payTotal) CKR(hipMemcpy(dp, h.pay, (size_t)h.payTotal, hipMemcpyHostToDevice));
    CKR(hipMemcpy(po, h.payOffs, tb, hipMemcpyHostToDevice));
    CKR(hipMemcpy(io, h.idxOffs, tb, hipMemcpyHostToDevice));
    *d = h; d->pay = dp; d->payOffs = po; d->idxOffs = io;
    return ULCX_OK;
}
// a whole host corpus, either layout: the above, its index and its block counts -> *d, the same corpus on the device
static int corpus_up(DevTmp &t, const UlcxCorpus &h, UlcxCorpus *d) {
    uint8_t *dp = nullptr; int32_t *dn = nullptr, *dcnt = nullptr; ulcx_index_entry *di = nullptr;
    *d = h;
    const int rc = h.ragged ? ragged_up(t, h, d) : payload_rows_up(t, h.nFiles, h.pay, h.payStride, h.payBytes, &dp, &dn);
    if (rc) return rc;
    if (!h.ragged) { d->pay = dp; d->payBytes = dn; }
    CKR(t.get(&dcnt, sizeof(int32_t) * (size_t)h.nFiles)); CKR(t.get(&di, sizeof(ulcx_index_entry) * (size_t)h.idxTotal));
    CKR(hipMemcpy(dcnt, h.indexBlocks, sizeof(int32_t) * (size_t)h.nFiles, hipMemcpyHostToDevice));
    if (h.idxTotal) CKR(hipMemcpy(di, h.index, sizeof(ulcx_index_entry) * (size_t)h.idxTotal, hipMemcpyHostToDevice));
    d->indexBlocks = dcnt; d->index = di;
    return ULCX_OK;
}

// ---- low-rate crops (include/ulc_amd_lowrate.h): what the synthesis of BlockSize >> lgD needs beside the object's own arrays, built
// by the first call at that ratio and kept - nothing is allocated by a later one
extern "C" int ulcx_lowrate_block(int BlockSize, int lgD) {
    if (lgD < 0 || lgD > 3 || !validate(1, BlockSize)) return 0;
    return validate(1, BlockSize >> lgD) ? BlockSize >> lgD : 0;
}
static int dec_low(ulcx_decoder *e, int lgD) {
    UlcxDecLow &l = e->low[lgD];
    if (l.ready) return ULCX_OK;
    const int BSr = e->BS >> lgD;
    int rc;
    if (!l.tables && (rc = ulcx_tables_build(&l.T, &l.tables, BSr, 44100, false))) return rc;
    dec_syn_geometry(e->C, BSr, &l.fastOK, &l.twInLds);      // the kernel pick of the REDUCED geometry
    if (l.fastOK) {
        bool want = true;
        if (const char *ev = getenv("ULCX_DSYN_SPLIT")) want = ev[0] != '0';
        UlcxDecCtx cs = e->ctx;
        cs.BS = BSr; cs.lgBS = ilog2i(BSr); cs.T = l.T; cs.fastOK = l.fastOK; cs.twInLds = l.twInLds;
        l.synSlots = want ? ulcx_dec_syn_slots(cs, ULCX_SYN_LOW, e->BS) : 0;
        if (l.synSlots > 0 && !l.lapScratch) {
            l.scratchRows = 4 * l.synSlots;
            if ((rc = dalloc(e->allocs, &l.lapScratch, (size_t)l.scratchRows * e->C * (BSr / 2), true))) return rc;
        }
    }
    l.ready = true;
    return ULCX_OK;
}
// lgD of a low-rate entry: refused outside 0 .. 3, or where the object's BlockSize >> lgD is no BlockSize
static int lowrate_bad(const char *who, const ulcx_decoder *e, int lgD) {
    if (lgD < 0 || lgD > 3) { refuse(who, "bad argument (lgD %d: 0 .. 3)", lgD); return 1; }
    if (e && !ulcx_lowrate_block(e->BS, lgD)) { refuse(who, "bad argument (lgD %d: BlockSize %d >> %d is below 256)", lgD, e->BS, lgD); return 1; }
    return 0;
}
// ---- crops (include/ulc_amd.h section 3): rows of a call that each name a file of a corpus.  The range synthesis enters every
// row from nothing, so the call needs no stream's state; what the synthesis leaves behind a row goes to the subset calls'
// shadow state (dec_shadow) and is never scattered back.
// the checks every crop entry makes, device or host pointers; the object comes last among them: every other refusal needs none
// (rowNull: one of the call's pointers beside the corpus's is NULL)
static int crops_checks(const char *who, const ulcx_decoder *e, const UlcxCorpus &g, bool rowNull, int n, int nBlocks) {
    if (rowNull || corpus_null(g)) { refuse(who, "bad argument (a NULL pointer)"); return 1; }
    if (n < 1) { refuse(who, "bad argument (n %d)", n); return 1; }
    if (g.nFiles < 1) { refuse(who, "bad argument (nFiles %d)", g.nFiles); return 1; }
    if (nBlocks < 1) { refuse(who, "bad argument (nBlocks is 1 .. maxBlocksPerCall - 1)"); return 1; }
    if (corpus_layout_bad(who, g)) return 1;
    if (!e) { refuse(who, "no decoder"); return 1; }
    if (n > e->B) { refuse(who, "bad argument (n %d: a call takes 1 .. nStreams = %d rows)", n, e->B); return 1; }
    if (nBlocks > e->maxK - 1) { refuse(who, "bad argument (nBlocks is 1 .. maxBlocksPerCall - 1)"); return 1; }
    return 0;
}
// the rows of a sample-crop call (ulcx_decode_crops_samples_*): d_first / d_count are not given, nBlocks is ulcx_crop_blocks(nSamples)
// (lgD > 0: a low-rate call, ulcx_decode_crops_lowrate_* - the rows count samples of the stream reduced by 1 << lgD)
// (part >= 0: a part call, ulcx_decode_crops_part_* - the output has ulcx_part_channels planes per row; else -1)
struct CropsSamples { const int64_t *start; const int32_t *len; int nSamples; int lgD; int part; };
// the outputs of a spectra call (ulcx_decode_crops_spectra_*) beside d_bits: coefficients instead of samples, and the window codes
struct CropsSpectra { float *coef; int32_t *wc; int flags; };
static int spectra_flags_bad(const char *who, int flags) {
    if (flags & ~ULCX_SPECTRA_LR) { refuse(who, "bad argument (flags 0x%x: 0 or ULCX_SPECTRA_LR)", (unsigned)flags); return 1; }
    return 0;
}
// the arguments of a distortion call (ulcx_decode_crops_distortion_*) in place of d_coef; the window codes travel in a CropsSpectra
struct CropsDistortion { const float *ref; int nRef, nRefBlocks; const int32_t *refRow, *refFirst; int nSeg; double *dist; };
// what a distortion call refuses beyond the spectra call, behind that call's own checks (the object is known by then)
static int distortion_bad(const char *who, const ulcx_decoder *e, const CropsDistortion &d, int flags, bool host) {
    const int W = d.nSeg > 0 ? e->BS / d.nSeg : 0;
    if (d.nSeg < 1 || d.nSeg > 64 || (d.nSeg & (d.nSeg - 1)) || W < 4) { refuse(who, "bad argument (nSeg %d: a power of two, 1 .. 64, with BlockSize / nSeg >= 4)", d.nSeg); return 1; }
    if (!host && (misaligned(who, "d_dist", d.dist, (int)sizeof(double)) || misaligned(who, "d_ref", d.ref, ULCX_ALIGN_PCM) ||
                  misaligned(who, "d_refRow", d.refRow, ULCX_ALIGN_WORD) || misaligned(who, "d_refFirst", d.refFirst, ULCX_ALIGN_WORD))) return 1;
    if (d.ref && (d.nRef < 1 || d.nRefBlocks < 1)) { refuse(who, "bad argument (nRef %d, nRefBlocks %d with a reference)", d.nRef, d.nRefBlocks); return 1; }
    if ((flags & ULCX_SPECTRA_LR) && ulcx_spec_arrays(e->BS) == 1) {
        refuse(who, "bad argument (flags: ULCX_SPECTRA_LR at BlockSize %d, where one unit array fills the LDS)", e->BS); return 1;
    }
    return 0;
}
// samp != NULL: a sample-crop call - the rows come from (start, len), the output is [n][nChan][nSamples] and needs its element's alignment only
// spec != NULL: a spectra call - d_pcm and d_pcm16 are NULL, the outputs are spec's [n][nChan][nBlocks][BlockSize] and [n][nBlocks]
// dist != NULL (with spec, whose coef is NULL): a distortion call - the sums of dist in place of the coefficients
static int decode_crops_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count,
                            int nBlocks, float *d_pcm, int16_t *d_pcm16, int32_t *d_bits, void *hipStream, const CropsSamples *samp = nullptr,
                            const CropsSpectra *spec = nullptr, const CropsDistortion *dist = nullptr) {
    if (spec && spectra_flags_bad(who, spec->flags)) return ULCX_ERR_ARG;
    const void *out = spec ? (spec->wc ? (dist ? (const void *)dist->dist : (const void *)spec->coef) : nullptr) : d_pcm ? (const void *)d_pcm : d_pcm16;
    const void *rows = samp ? (const void *)samp->start : d_first;
    if (crops_checks(who, e, g, !d_file || !rows || !out || !d_bits, n, nBlocks)) return ULCX_ERR_ARG;
    if (corpus_misaligned(who, g) || misaligned(who, "d_file", d_file, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_first", d_first, ULCX_ALIGN_WORD) || misaligned(who, "d_count", d_count, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    if (spec && (misaligned(who, "d_coef", spec->coef, ULCX_ALIGN_PCM) || misaligned(who, "d_wc", spec->wc, ULCX_ALIGN_WORD))) return ULCX_ERR_ARG;
    if (spec && (long long)n * nBlocks * ((e->C + 1) / 2) > 0x7FFFFFFFLL) return refuse(who, "bad argument (n x nBlocks x channel pairs exceeds a grid)");
    if (dist && distortion_bad(who, e, *dist, spec->flags, false)) return ULCX_ERR_ARG;
    // (a plane of a sample crop starts at any sample: the kernels use wider stores only where the address allows them)
    if (samp ? (misaligned(who, "d_start", samp->start, ULCX_ALIGN_OFFS) || misaligned(who, "d_len", samp->len, ULCX_ALIGN_WORD) ||
                misaligned(who, "d_pcm", d_pcm, (int)sizeof(float)) || misaligned(who, "d_pcm16", d_pcm16, (int)sizeof(int16_t)))
             : (misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) || misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_PCM16))) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    int rc = dec_shadow(e);
    if (!rc && samp && samp->lgD > 0) rc = dec_low(e, samp->lgD);
    if (rc) return rc;
    UlcxDecCtx c = e->ctx;
    c.B = n; c.K = nBlocks + 1; c.slot = 0; c.in = g.pay; c.inBytes = g.payTotal; c.pcm = d_pcm; c.pcm16 = d_pcm16;
    c.bits = e->bitsScr; c.bitsOut = d_bits;
    c.packed = 1; c.range = 1; c.rFirst = d_first;
    c.lap = e->subLap[0]; c.lastSub = e->subLastSub[0]; c.seed = e->subSeed[0]; c.dead = e->subDead[0]; c.packOff = e->subPackOff;
    UlcxDecAux crop = {};
    crop.kind = dist ? ULCX_DEC_DISTORTION : spec ? ULCX_DEC_SPECTRA : !samp ? ULCX_DEC_CROPS : samp->part >= 0 ? ULCX_DEC_PART : samp->lgD > 0 ? ULCX_DEC_LOWRATE : ULCX_DEC_SAMPLES;
    crop.corpus = g; crop.cropFile = d_file; crop.cropCount = d_count;
    if (samp) {
        crop.samp = { samp->start, samp->len, samp->nSamples, e->sampRows, e->sampRows + e->B, e->sampRows + 2 * (size_t)e->B, e->sampRows + 3 * (size_t)e->B };
        c.rFirst = crop.samp.first; crop.cropCount = crop.samp.count;
        if (samp->lgD > 0) {
            const UlcxDecLow &l = e->low[samp->lgD];
            crop.low = { samp->lgD, l.T, l.fastOK, l.twInLds, l.lapScratch };
        }
        if (samp->part >= 0) {
            // at full rate the object's own tables and pick serve; no cut: the lapping state is the rows' own shadow rows
            if (samp->lgD == 0) crop.low = { 0, e->ctx.T, e->ctx.fastOK, e->ctx.twInLds, nullptr };
            crop.low.lapScratch = nullptr;
            crop.part = { samp->part, ulcx_part_channels(e->C, samp->part) };
        }
    }
    if (spec) crop.spec = { spec->coef, spec->wc, (spec->flags & ULCX_SPECTRA_LR) ? 1 : 0 };
    if (dist) crop.dist = { dist->dist, dist->ref, dist->nRef, dist->nRefBlocks, dist->nSeg, dist->refRow, dist->refFirst };
    int set = 0;
    rc = dec_launch(e, c, (hipStream_t)hipStream, &set, &crop);
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    return rc;
}
extern "C" int ulcx_decode_crops_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                     const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                     int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                     float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_crops_any("ulcx_decode_crops_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                           const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                           int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                           int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return decode_crops_any("ulcx_decode_crops_dev_pcm16", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, d_pcm16, d_bits, hipStream);
}
// what a host form leaves of a spectra call beside the crop results: the window codes (hspec: the HOST outputs, flags as given)
static int spectra_wc_down(const int32_t *d_wc, size_t NB, int32_t *h_wc) {
    CKR(hipMemcpy(h_wc, d_wc, sizeof(int32_t) * NB, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
// the host forms, either layout: ulcx_decode_crops[_ragged]_host (h_pcm), ulcx_decode_crops_spectra[_ragged]_host (hspec: h_pcm
// is its coefficients) and ulcx_decode_crops_distortion[_ragged]_host (hspec and hdist, all HOST pointers: h_pcm is NULL)
static int crops_host_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count,
                          int nBlocks, float *h_pcm, int32_t *h_bits, const CropsSpectra *hspec = nullptr, const CropsDistortion *hdist = nullptr) {
    if (hspec && spectra_flags_bad(who, hspec->flags)) return ULCX_ERR_ARG;
    if (crops_checks(who, e, g, !h_file || !h_first || (hspec && !hspec->wc) || !(hdist ? (const void *)hdist->dist : (const void *)h_pcm) || !h_bits, n, nBlocks)) return ULCX_ERR_ARG;
    if (hdist && distortion_bad(who, e, *hdist, hspec->flags, true)) return ULCX_ERR_ARG;
    // what the device forms cannot refuse: a ragged corpus's tables, then the rows
    if (g.ragged && ragged_tables_bad(who, g)) return ULCX_ERR_ARG;
    for (int i = 0; i < n; i++) {
        long long nI;
        if (host_row_file(who, g, i, h_file[i], &nI)) return ULCX_ERR_ARG;
        if (h_first[i] < 0 || h_first[i] > nI) return refuse(who, "row %d starts at block %d of a file of %lld", i, (int)h_first[i], nI);
        if (h_count && h_count[i] < 0) return refuse(who, "row %d wants %d blocks", i, (int)h_count[i]);
    }
    CKR(hipSetDevice(e->device));
    const size_t NB = (size_t)n * nBlocks;
    DevTmp t; UlcxCorpus d; int32_t *dfile = nullptr, *df = nullptr, *dwant = nullptr, *dbits = nullptr; float *dpcm = nullptr;
    int rc = corpus_up(t, g, &d);
    if (rc) return rc;
    CKR(t.get(&dfile, sizeof(int32_t) * n)); CKR(t.get(&df, sizeof(int32_t) * n));
    if (!hdist) CKR(t.get(&dpcm, sizeof(float) * NB * (size_t)e->C * e->BS));
    CKR(t.get(&dbits, sizeof(int32_t) * NB));
    CKR(hipMemcpy(dfile, h_file, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    CKR(hipMemcpy(df, h_first, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (h_count) { CKR(t.get(&dwant, sizeof(int32_t) * n)); CKR(hipMemcpy(dwant, h_count, sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
    CropsSpectra ds = {};
    if (hspec) { ds.coef = dpcm; ds.flags = hspec->flags; CKR(t.get(&ds.wc, sizeof(int32_t) * NB)); }
    CropsDistortion dd = {};
    const size_t nDist = NB * (size_t)e->C * (hdist ? hdist->nSeg : 0) * 3;
    if (hdist) {                                                  // the reference and its two tables up, the sums' buffer
        dd = *hdist; dd.ref = nullptr; dd.refRow = dd.refFirst = nullptr;
        CKR(t.get(&dd.dist, sizeof(double) * nDist));
        if (hdist->ref) {
            const size_t nRefF = (size_t)hdist->nRef * e->C * hdist->nRefBlocks * e->BS;
            float *dref = nullptr; int32_t *drow = nullptr, *dfirst = nullptr;
            CKR(t.get(&dref, sizeof(float) * nRefF)); CKR(hipMemcpy(dref, hdist->ref, sizeof(float) * nRefF, hipMemcpyHostToDevice));
            if (hdist->refRow) { CKR(t.get(&drow, sizeof(int32_t) * n)); CKR(hipMemcpy(drow, hdist->refRow, sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
            if (hdist->refFirst) { CKR(t.get(&dfirst, sizeof(int32_t) * n)); CKR(hipMemcpy(dfirst, hdist->refFirst, sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
            dd.ref = dref; dd.refRow = drow; dd.refFirst = dfirst;
        }
    }
    rc = decode_crops_any(who, e, d, n, dfile, df, dwant, nBlocks, hspec ? nullptr : dpcm, nullptr, dbits, nullptr, nullptr, hspec ? &ds : nullptr, hdist ? &dd : nullptr);
    if (!rc && hdist) {
        CKR(hipDeviceSynchronize());
        CKR(hipMemcpy(hdist->dist, dd.dist, sizeof(double) * nDist, hipMemcpyDeviceToHost));
        CKR(hipMemcpy(h_bits, dbits, sizeof(int32_t) * NB, hipMemcpyDeviceToHost));
    } else if (!rc) rc = dec_results_down(e, dpcm, dbits, NB, h_pcm, h_bits);
    return (rc || !hspec) ? rc : spectra_wc_down(ds.wc, NB, hspec->wc);
}
extern "C" int ulcx_decode_crops_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                      const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                      int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks,
                                      float *h_pcm, int32_t *h_bits) {
    return crops_host_any("ulcx_decode_crops_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, h_pcm, h_bits);
}
// ulcx_index_packed_* with a row count of its own: k_dindex over nRows (geometry and tables are all that is read of the object)
static int index_rows_packed_any(const char *who, ulcx_decoder *e, int nRows, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                 int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream) {
    if (!d_payload || !d_payloadBytes || !d_index || !d_nBlocks || nRows < 1 || payloadStride < 1 || maxBlocks < 1) return refuse(who, "bad argument");
    if (!e) return refuse(who, "no decoder");
    if (misaligned(who, "d_payloadBytes", d_payloadBytes, ULCX_ALIGN_WORD) || misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_nBlocks", d_nBlocks, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.B = nRows; c.in = d_payload; c.packed = 1; c.payStride = payloadStride; c.payBytes = d_payloadBytes;
    c.inBytes = (long long)nRows * payloadStride;
    return ulcx_index_launch(c, maxBlocks, d_index, d_nBlocks, (hipStream_t)hipStream);
}
extern "C" int ulcx_index_packed_rows_dev(ulcx_decoder *e, int nRows, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                          int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream) {
    return index_rows_packed_any("ulcx_index_packed_rows_dev", e, nRows, d_payload, payloadStride, d_payloadBytes, maxBlocks, d_index, d_nBlocks, hipStream);
}
extern "C" int ulcx_index_packed_rows_host(ulcx_decoder *e, int nRows, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                           int maxBlocks, ulcx_index_entry *h_index, int32_t *h_nBlocks) {
    const char *who = "ulcx_index_packed_rows_host";
    if (!e || !h_payload || !h_payloadBytes || !h_index || !h_nBlocks || nRows < 1 || payloadStride < 1 || maxBlocks < 1) return refuse(who, "bad argument");
    CKR(hipSetDevice(e->device));
    DevTmp t; uint8_t *dp = nullptr; int32_t *dn = nullptr, *dcnt = nullptr; ulcx_index_entry *di = nullptr;
    const size_t nEnt = (size_t)nRows * ((size_t)maxBlocks + 1);
    int rc = payload_rows_up(t, nRows, h_payload, payloadStride, h_payloadBytes, &dp, &dn);
    if (rc) return rc;
    CKR(t.get(&dcnt, sizeof(int32_t) * (size_t)nRows)); CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt));
    if ((rc = index_rows_packed_any(who, e, nRows, dp, payloadStride, dn, maxBlocks, di, dcnt, nullptr))) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_index, di, sizeof(ulcx_index_entry) * nEnt, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_nBlocks, dcnt, sizeof(int32_t) * (size_t)nRows, hipMemcpyDeviceToHost));
    return ULCX_OK;
}

// ---- crops of a ragged corpus (include/ulc_amd.h section 3): the crop family's bodies on a corpus whose files are found through offset tables.
extern "C" int ulcx_decode_crops_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                            const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                            int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                            float *d_pcm, int32_t *d_bits, void *hipStream) {
    return decode_crops_any("ulcx_decode_crops_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_ragged_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                  const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                  int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                                  int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return decode_crops_any("ulcx_decode_crops_ragged_dev_pcm16", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, d_pcm16, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                             const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                             int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks,
                                             float *h_pcm, int32_t *h_bits) {
    return crops_host_any("ulcx_decode_crops_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, h_pcm, h_bits);
}
// ---- spectra (include/ulc_amd.h section 3): the crop families' bodies, ending in the dequantised coefficients instead of samples.
extern "C" int ulcx_window_subblocks(int BlockSize, int wc, int sizes[4]) {
    // a code a block can carry (ulcDecoder.c:211-216): the first nybble, and the second one only behind a first with bit 3 set
    if (!validate(1, BlockSize) || wc < 0 || wc > 0xFF || (!(wc & 8) && (wc >> 4) != 1)) return 0;
    unsigned pat = ulcx_pattern(wc);
    int nsub = 0;
    do {
        const int S = BlockSize >> (pat & 7);
        if (sizes) sizes[nsub] = S;
        nsub++;
        if (S == BlockSize) break;                                // ulcDecoder.c:242-245
    } while (pat >>= 4);
    if (sizes) for (int j = nsub; j < 4; j++) sizes[j] = 0;
    return nsub;
}
extern "C" int ulcx_decode_crops_spectra_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                             const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                             int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks, int flags,
                                             float *d_coef, int32_t *d_wc, int32_t *d_bits, void *hipStream) {
    const CropsSpectra sp = { d_coef, d_wc, flags };
    return decode_crops_any("ulcx_decode_crops_spectra_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, nullptr, d_bits, hipStream, nullptr, &sp);
}
extern "C" int ulcx_decode_crops_spectra_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                    const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                    int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks, int flags,
                                                    float *d_coef, int32_t *d_wc, int32_t *d_bits, void *hipStream) {
    const CropsSpectra sp = { d_coef, d_wc, flags };
    return decode_crops_any("ulcx_decode_crops_spectra_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, nullptr, d_bits, hipStream, nullptr, &sp);
}
extern "C" int ulcx_decode_crops_spectra_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                              const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                              int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks, int flags,
                                              float *h_coef, int32_t *h_wc, int32_t *h_bits) {
    const CropsSpectra sp = { h_coef, h_wc, flags };
    return crops_host_any("ulcx_decode_crops_spectra_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, h_coef, h_bits, &sp);
}
extern "C" int ulcx_decode_crops_spectra_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                                     const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                                     int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks, int flags,
                                                     float *h_coef, int32_t *h_wc, int32_t *h_bits) {
    const CropsSpectra sp = { h_coef, h_wc, flags };
    return crops_host_any("ulcx_decode_crops_spectra_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, h_coef, h_bits, &sp);
}
// ---- distortion (include/ulc_amd.h section 3): the spectra calls' bodies, ending in the sums against reference planes instead of the coefficients.
extern "C" int ulcx_decode_crops_distortion_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                                const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                                int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                                const float *d_ref, int nRef, int nRefBlocks, const int32_t *d_refRow, const int32_t *d_refFirst, int nSeg, int flags,
                                                double *d_dist, int32_t *d_wc, int32_t *d_bits, void *hipStream) {
    const CropsSpectra sp = { nullptr, d_wc, flags };
    const CropsDistortion di = { d_ref, nRef, nRefBlocks, d_refRow, d_refFirst, nSeg, d_dist };
    return decode_crops_any("ulcx_decode_crops_distortion_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, nullptr, d_bits, hipStream, nullptr, &sp, &di);
}
extern "C" int ulcx_decode_crops_distortion_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                       const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                       int n, const int32_t *d_file, const int32_t *d_first, const int32_t *d_count, int nBlocks,
                                                       const float *d_ref, int nRef, int nRefBlocks, const int32_t *d_refRow, const int32_t *d_refFirst, int nSeg, int flags,
                                                       double *d_dist, int32_t *d_wc, int32_t *d_bits, void *hipStream) {
    const CropsSpectra sp = { nullptr, d_wc, flags };
    const CropsDistortion di = { d_ref, nRef, nRefBlocks, d_refRow, d_refFirst, nSeg, d_dist };
    return decode_crops_any("ulcx_decode_crops_distortion_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                            n, d_file, d_first, d_count, nBlocks, nullptr, nullptr, d_bits, hipStream, nullptr, &sp, &di);
}
extern "C" int ulcx_decode_crops_distortion_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                                 const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                                 int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks,
                                                 const float *h_ref, int nRef, int nRefBlocks, const int32_t *h_refRow, const int32_t *h_refFirst, int nSeg, int flags,
                                                 double *h_dist, int32_t *h_wc, int32_t *h_bits) {
    const CropsSpectra sp = { nullptr, h_wc, flags };
    const CropsDistortion di = { h_ref, nRef, nRefBlocks, h_refRow, h_refFirst, nSeg, h_dist };
    return crops_host_any("ulcx_decode_crops_distortion_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, nullptr, h_bits, &sp, &di);
}
extern "C" int ulcx_decode_crops_distortion_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                                        const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                                        int n, const int32_t *h_file, const int32_t *h_first, const int32_t *h_count, int nBlocks,
                                                        const float *h_ref, int nRef, int nRefBlocks, const int32_t *h_refRow, const int32_t *h_refFirst, int nSeg, int flags,
                                                        double *h_dist, int32_t *h_wc, int32_t *h_bits) {
    const CropsSpectra sp = { nullptr, h_wc, flags };
    const CropsDistortion di = { h_ref, nRef, nRefBlocks, h_refRow, h_refFirst, nSeg, h_dist };
    return crops_host_any("ulcx_decode_crops_distortion_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                          n, h_file, h_first, h_count, nBlocks, nullptr, h_bits, &sp, &di);
}
// ---- sample crops (include/ulc_amd.h section 3): the crop families' bodies with rows given in samples and the output channels-first.
extern "C" int ulcx_crop_blocks(int BlockSize, int nSamples) {
    if (BlockSize < 1 || nSamples < 1) return 0;
    const long long nB = 1 + ((long long)nSamples + BlockSize - 2) / BlockSize;
    return nB > 0x7FFFFFFFLL ? 0x7FFFFFFF : (int)nB;
}
// nSamples of a sample-crop entry -> the blocks per row the crop body is called with (checked there against maxBlocksPerCall - 1);
// 0: refused here.  Without an object the count is 1: the body then refuses the call for the object's absence, or for what it
// checks before that.
// (lgD: a low-rate entry - the blocks are those of BlockSize >> lgD)
static int samples_blocks(const char *who, const ulcx_decoder *e, int nSamples, int lgD = 0) {
    if (nSamples < 1) { refuse(who, "bad argument (nSamples %d)", nSamples); return 0; }
    if (!e) return 1;
    const int nB = ulcx_crop_blocks(e->BS >> lgD, nSamples);
    if (nB > e->maxK - 1) { refuse(who, "bad argument (nSamples %d touches up to %d blocks; a row has maxBlocksPerCall - 1 = %d)", nSamples, nB, e->maxK - 1); return 0; }
    return nB;
}
static int crops_samples_dev_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                 int nSamples, float *d_pcm, int16_t *d_pcm16, int32_t *d_bits, void *hipStream, int lgD = 0, int part = -1) {
    if (lowrate_bad(who, e, lgD)) return ULCX_ERR_ARG;
    const int nB = samples_blocks(who, e, nSamples, lgD);
    if (!nB) return ULCX_ERR_ARG;
    const CropsSamples sm = { d_start, d_len, nSamples, lgD, part };
    return decode_crops_any(who, e, g, n, d_file, nullptr, nullptr, nB, d_pcm, d_pcm16, d_bits, hipStream, &sm);
}
extern "C" int ulcx_decode_crops_samples_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                             const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                             int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples,
                                             float *d_pcm, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_samples_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_samples_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                                   const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                                   int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples,
                                                   int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_samples_dev_pcm16", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_samples_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                    const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                    int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples,
                                                    float *d_pcm, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_samples_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream);
}
extern "C" int ulcx_decode_crops_samples_ragged_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                          const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                          int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples,
                                                          int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_samples_ragged_dev_pcm16", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream);
}
// what the device forms cannot refuse of row i, which names a file of nI indexed blocks
static int sample_row_bad(const char *who, int i, int BS, long long nI, long long start, const int32_t *h_len) {
    if (start < 0 || start > nI * BS) { refuse(who, "row %d starts at sample %lld of a file of %lld blocks of %d", i, start, nI, BS); return 1; }
    if (h_len && h_len[i] < 0) { refuse(who, "row %d wants %d samples", i, (int)h_len[i]); return 1; }
    return 0;
}
// the rows of a host form up, its output buffers, and after the call the results down: [n][nChan][nSamples] samples, [n][nB] sizes
struct SampleStage { int32_t *file = nullptr, *len = nullptr, *bits = nullptr; int64_t *start = nullptr; float *pcm = nullptr; };
// (planes: the planes of an output row - nChan, or a part call's ulcx_part_channels)
static int sample_rows_up(DevTmp &t, int planes, int n, int nB, int nSamples, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, SampleStage *g) {
    CKR(t.get(&g->file, sizeof(int32_t) * n)); CKR(t.get(&g->start, sizeof(int64_t) * n));
    CKR(t.get(&g->pcm, sizeof(float) * (size_t)n * planes * (size_t)nSamples)); CKR(t.get(&g->bits, sizeof(int32_t) * (size_t)n * nB));
    CKR(hipMemcpy(g->file, h_file, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    CKR(hipMemcpy(g->start, h_start, sizeof(int64_t) * n, hipMemcpyHostToDevice));
    if (h_len) { CKR(t.get(&g->len, sizeof(int32_t) * n)); CKR(hipMemcpy(g->len, h_len, sizeof(int32_t) * n, hipMemcpyHostToDevice)); }
    return ULCX_OK;
}
static int sample_results_down(int planes, const SampleStage &g, int n, int nB, int nSamples, float *h_pcm, int32_t *h_bits) {
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_pcm, g.pcm, sizeof(float) * (size_t)n * planes * (size_t)nSamples, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_bits, g.bits, sizeof(int32_t) * (size_t)n * nB, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
// the host forms, either layout
static int crops_samples_host_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                  int nSamples, float *h_pcm, int32_t *h_bits, int lgD = 0, int part = -1) {
    if (lowrate_bad(who, e, lgD)) return ULCX_ERR_ARG;
    const int nB = samples_blocks(who, e, nSamples, lgD);
    if (!nB) return ULCX_ERR_ARG;
    if (crops_checks(who, e, g, !h_file || !h_start || !h_pcm || !h_bits, n, nB)) return ULCX_ERR_ARG;
    if (g.ragged && ragged_tables_bad(who, g)) return ULCX_ERR_ARG;
    for (int i = 0; i < n; i++) {
        long long nI;
        if (host_row_file(who, g, i, h_file[i], &nI)) return ULCX_ERR_ARG;
        if (sample_row_bad(who, i, e->BS >> lgD, nI < 0 ? 0 : nI, h_start[i], h_len)) return ULCX_ERR_ARG;
    }
    CKR(hipSetDevice(e->device));
    DevTmp t; UlcxCorpus d; SampleStage sg;
    const int planes = part >= 0 ? ulcx_part_channels(e->C, part) : e->C;
    int rc = corpus_up(t, g, &d);
    if (!rc) rc = sample_rows_up(t, planes, n, nB, nSamples, h_file, h_start, h_len, &sg);
    if (rc) return rc;
    const CropsSamples sm = { sg.start, sg.len, nSamples, lgD, part };
    rc = decode_crops_any(who, e, d, n, sg.file, nullptr, nullptr, nB, sg.pcm, nullptr, sg.bits, nullptr, &sm);
    return rc ? rc : sample_results_down(planes, sg, n, nB, nSamples, h_pcm, h_bits);
}
extern "C" int ulcx_decode_crops_samples_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                              const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                              int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples,
                                              float *h_pcm, int32_t *h_bits) {
    return crops_samples_host_any("ulcx_decode_crops_samples_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits);
}
extern "C" int ulcx_decode_crops_samples_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                                     const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                                     int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples,
                                                     float *h_pcm, int32_t *h_bits) {
    return crops_samples_host_any("ulcx_decode_crops_samples_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits);
}
// ---- low-rate sample crops (include/ulc_amd_lowrate.h): the sample-crop bodies with one further argument
extern "C" int ulcx_decode_crops_lowrate_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                             const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                             int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD,
                                             float *d_pcm, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_lowrate_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream, lgD);
}
extern "C" int ulcx_decode_crops_lowrate_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                                   const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                                   int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD,
                                                   int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_lowrate_dev_pcm16", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream, lgD);
}
extern "C" int ulcx_decode_crops_lowrate_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                              const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                              int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples, int lgD,
                                              float *h_pcm, int32_t *h_bits) {
    return crops_samples_host_any("ulcx_decode_crops_lowrate_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits, lgD);
}
extern "C" int ulcx_decode_crops_lowrate_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                    const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                    int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD,
                                                    float *d_pcm, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_lowrate_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream, lgD);
}
extern "C" int ulcx_decode_crops_lowrate_ragged_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                          const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                          int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD,
                                                          int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    return crops_samples_dev_any("ulcx_decode_crops_lowrate_ragged_dev_pcm16", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream, lgD);
}
extern "C" int ulcx_decode_crops_lowrate_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                                     const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                                     int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples, int lgD,
                                                     float *h_pcm, int32_t *h_bits) {
    return crops_samples_host_any("ulcx_decode_crops_lowrate_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits, lgD);
}
// ---- mid and side crops (include/ulc_amd_part.h): the low-rate bodies with one further argument - the coded channels part, part + 2, ...
// of every row, each as it stands in front of the un-mix, into (nChan + 1 - part) / 2 planes
extern "C" int ulcx_part_channels(int nChan, int part) {
    if (nChan < 1 || nChan > 255 || part < ULCX_PART_MID || part > ULCX_PART_SIDE) return 0;
    return (nChan + 1 - part) / 2;
}
// part of a part entry: refused outside 0 .. 1, or where the object's channels have no such part (the side of a mono corpus)
static int part_bad(const char *who, const ulcx_decoder *e, int part) {
    if (part < ULCX_PART_MID || part > ULCX_PART_SIDE) { refuse(who, "bad argument (part %d: ULCX_PART_MID or ULCX_PART_SIDE)", part); return 1; }
    if (e && !ulcx_part_channels(e->C, part)) { refuse(who, "bad argument (part %d: %d channel(s) have no side)", part, e->C); return 1; }
    return 0;
}
extern "C" int ulcx_decode_crops_part_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                          const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                          int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD, int part,
                                          float *d_pcm, int32_t *d_bits, void *hipStream) {
    const char *who = "ulcx_decode_crops_part_dev";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_dev_any(who, e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream, lgD, part);
}
extern "C" int ulcx_decode_crops_part_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                                const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                                int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD, int part,
                                                int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    const char *who = "ulcx_decode_crops_part_dev_pcm16";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_dev_any(who, e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream, lgD, part);
}
extern "C" int ulcx_decode_crops_part_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                           const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                           int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples, int lgD, int part,
                                           float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_crops_part_host";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_host_any(who, e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits, lgD, part);
}
extern "C" int ulcx_decode_crops_part_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                 const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                 int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD, int part,
                                                 float *d_pcm, int32_t *d_bits, void *hipStream) {
    const char *who = "ulcx_decode_crops_part_ragged_dev";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_dev_any(who, e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, d_pcm, nullptr, d_bits, hipStream, lgD, part);
}
extern "C" int ulcx_decode_crops_part_ragged_dev_pcm16(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                       const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                                       int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len, int nSamples, int lgD, int part,
                                                       int16_t *d_pcm16, int32_t *d_bits, void *hipStream) {
    const char *who = "ulcx_decode_crops_part_ragged_dev_pcm16";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_dev_any(who, e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                                 n, d_file, d_start, d_len, nSamples, nullptr, d_pcm16, d_bits, hipStream, lgD, part);
}
extern "C" int ulcx_decode_crops_part_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                                  const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                                  int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len, int nSamples, int lgD, int part,
                                                  float *h_pcm, int32_t *h_bits) {
    const char *who = "ulcx_decode_crops_part_ragged_host";
    if (part_bad(who, e, part)) return ULCX_ERR_ARG;
    return crops_samples_host_any(who, e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                                  n, h_file, h_start, h_len, nSamples, h_pcm, h_bits, lgD, part);
}
// ---- synthesis from spectra (include/ulc_amd.h section 3): the decoder's inverse transform on caller-held planes.  The range
// synthesis of a crop call without any walk in front: the call runs on the shadow state as the crop calls do (dec_shadow; nothing
// is scattered back), on the object's per-block rows, under the range call's launch plan for n rows of nOut blocks.
// The checks of every synth entry, device or host pointers; *nOut: the blocks per row that come out
static int synth_args_bad(const char *who, const ulcx_decoder *e, int n, int nBlocks, int flags, const void *coef, const void *wc, const void *pcm, const void *live, int *nOut) {
    if (flags & ~(ULCX_SPECTRA_LR | ULCX_SYNTH_WARM)) { refuse(who, "bad argument (flags 0x%x: ULCX_SPECTRA_LR, ULCX_SYNTH_WARM)", (unsigned)flags); return 1; }
    if (!coef || !wc || !pcm || !live) { refuse(who, "bad argument (a NULL pointer)"); return 1; }
    if (n < 1) { refuse(who, "bad argument (n %d)", n); return 1; }
    if (!e) { refuse(who, "no decoder"); return 1; }
    if (n > e->B) { refuse(who, "bad argument (n %d: a call takes 1 .. nStreams = %d rows)", n, e->B); return 1; }
    const int warm = (flags & ULCX_SYNTH_WARM) ? 1 : 0;
    if (nBlocks < 1 + warm || nBlocks - warm > e->maxK - 1) {
        refuse(who, "bad argument (nBlocks %d: %d .. %d%s)", nBlocks, 1 + warm, e->maxK - 1 + warm, warm ? " with the plane in front" : "");
        return 1;
    }
    if ((long long)(nBlocks - warm) * e->BS > 0x7FFFFFFFLL) { refuse(who, "bad argument (a row of %d blocks exceeds 2^31 samples)", nBlocks - warm); return 1; }
    *nOut = nBlocks - warm;
    return 0;
}
static int synth_spectra_any(const char *who, ulcx_decoder *e, int n, int nBlocks, int flags, const float *d_coef, const int32_t *d_wc,
                             float *d_pcm, int16_t *d_pcm16, int32_t *d_live, void *hipStream) {
    int nOut = 0;
    if (synth_args_bad(who, e, n, nBlocks, flags, d_coef, d_wc, d_pcm ? (const void *)d_pcm : d_pcm16, d_live, &nOut)) return ULCX_ERR_ARG;
    if (misaligned(who, "d_coef", d_coef, ULCX_ALIGN_PCM) || misaligned(who, "d_wc", d_wc, ULCX_ALIGN_WORD) || misaligned(who, "d_pcm", d_pcm, ULCX_ALIGN_PCM) ||
        misaligned(who, "d_pcm16", d_pcm16, ULCX_ALIGN_WORD) || misaligned(who, "d_live", d_live, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    // (d_pcm16 at 4 bytes: the sample store mode pairs its stores only where a plane's address allows it)
    CKR(hipSetDevice(e->device));
    int rc = dec_shadow(e);
    if (rc) return rc;
    UlcxDecCtx c = e->ctx;
    c.B = n; c.K = nOut + 1; c.slot = 0; c.in = nullptr; c.inBytes = 0; c.pcm = d_pcm; c.pcm16 = d_pcm16;
    c.bits = e->bitsScr; c.bitsOut = d_live;
    c.packed = 1; c.payStride = 0; c.payBytes = nullptr;
    c.range = 1; c.rIndex = nullptr; c.rIndexStride = 0; c.rIndexBlocks = nullptr; c.rFirst = nullptr;
    c.lap = e->subLap[0]; c.lastSub = e->subLastSub[0]; c.seed = e->subSeed[0]; c.dead = e->subDead[0]; c.packOff = e->subPackOff;
    UlcxDecAux syn = {}; syn.kind = ULCX_DEC_SYNTH;
    syn.syn = { d_coef, d_wc, nBlocks, (flags & ULCX_SPECTRA_LR) ? 1 : 0 };
    syn.samp.nSamples = nOut * e->BS; syn.samp.skip = e->sampRows + 2 * (size_t)e->B; syn.samp.lenC = e->sampRows + 3 * (size_t)e->B;
    int set = 0;
    rc = dec_launch(e, c, (hipStream_t)hipStream, &set, &syn);
    e->evRecorded = (rc == ULCX_OK) && e->timing;
    return rc;
}
extern "C" int ulcx_synth_spectra_dev(ulcx_decoder *e, int n, int nBlocks, int flags, const float *d_coef, const int32_t *d_wc, float *d_pcm, int32_t *d_live,
                                      void *hipStream) {
    return synth_spectra_any("ulcx_synth_spectra_dev", e, n, nBlocks, flags, d_coef, d_wc, d_pcm, nullptr, d_live, hipStream);
}
extern "C" int ulcx_synth_spectra_dev_pcm16(ulcx_decoder *e, int n, int nBlocks, int flags, const float *d_coef, const int32_t *d_wc, int16_t *d_pcm16, int32_t *d_live,
                                            void *hipStream) {
    return synth_spectra_any("ulcx_synth_spectra_dev_pcm16", e, n, nBlocks, flags, d_coef, d_wc, nullptr, d_pcm16, d_live, hipStream);
}
extern "C" int ulcx_synth_spectra_host(ulcx_decoder *e, int n, int nBlocks, int flags, const float *h_coef, const int32_t *h_wc, float *h_pcm, int32_t *h_live) {
    const char *who = "ulcx_synth_spectra_host";
    int nOut = 0;
    if (synth_args_bad(who, e, n, nBlocks, flags, h_coef, h_wc, h_pcm, h_live, &nOut)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t nCoef = (size_t)n * e->C * (size_t)nBlocks * e->BS, nWc = (size_t)n * nBlocks, NB = (size_t)n * nOut;
    DevTmp t; float *dcoef = nullptr, *dpcm = nullptr; int32_t *dwc = nullptr, *dlive = nullptr;
    CKR(t.get(&dcoef, sizeof(float) * nCoef)); CKR(t.get(&dwc, sizeof(int32_t) * nWc));
    CKR(t.get(&dpcm, sizeof(float) * NB * (size_t)e->C * e->BS)); CKR(t.get(&dlive, sizeof(int32_t) * NB));
    CKR(hipMemcpy(dcoef, h_coef, sizeof(float) * nCoef, hipMemcpyHostToDevice));
    CKR(hipMemcpy(dwc, h_wc, sizeof(int32_t) * nWc, hipMemcpyHostToDevice));
    const int rc = synth_spectra_any(who, e, n, nBlocks, flags, dcoef, dwc, dpcm, nullptr, dlive, nullptr);
    return rc ? rc : dec_results_down(e, dpcm, dlive, NB, h_pcm, h_live);
}
// ulcx_index_packed_rows_* for files back to back: k_dindex_ragged over the files of g, whose index is the output and which has no
// block counts yet (geometry and tables are all that is read of the object)
static int index_ragged_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, ulcx_index_entry *d_index, int32_t *d_nBlocks, void *hipStream) {
    if (!g.pay || !g.payOffs || !d_index || !g.idxOffs || !d_nBlocks || g.nFiles < 1 || g.payTotal < 0 || g.idxTotal < 0) return refuse(who, "bad argument");
    if (!e) return refuse(who, "no decoder");
    if (misaligned(who, "d_payloadOffs", g.payOffs, ULCX_ALIGN_OFFS) || misaligned(who, "d_indexOffs", g.idxOffs, ULCX_ALIGN_OFFS) ||
        misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) || misaligned(who, "d_nBlocks", d_nBlocks, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.B = g.nFiles; c.in = g.pay; c.packed = 1; c.payStride = 0; c.payBytes = nullptr;
    c.inBytes = g.payTotal;
    return ulcx_index_ragged_launch(c, g.payOffs, g.idxOffs, g.idxTotal, d_index, d_nBlocks, (hipStream_t)hipStream);
}
extern "C" int ulcx_index_packed_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                            ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, int32_t *d_nBlocks, void *hipStream) {
    return index_ragged_any("ulcx_index_packed_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, nullptr),
                            d_index, d_nBlocks, hipStream);
}
// (h_index is read as well as written: the entries between and behind the rows go back as they came)
extern "C" int ulcx_index_packed_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                             ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, int32_t *h_nBlocks) {
    const char *who = "ulcx_index_packed_ragged_host";
    const UlcxCorpus g = ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, nullptr);
    if (!h_payload || !h_payloadOffs || !h_index || !h_indexOffs || !h_nBlocks || nFiles < 1 || payloadTotal < 0 || indexTotal < 0) return refuse(who, "bad argument");
    if (!e) return refuse(who, "no decoder");
    if (ragged_tables_bad(who, g)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    DevTmp t; int32_t *dcnt = nullptr; ulcx_index_entry *di = nullptr; UlcxCorpus d;
    int rc = ragged_up(t, g, &d);
    if (rc) return rc;
    CKR(t.get(&dcnt, sizeof(int32_t) * (size_t)nFiles)); CKR(t.get(&di, sizeof(ulcx_index_entry) * (size_t)indexTotal));
    if (indexTotal) CKR(hipMemcpy(di, h_index, sizeof(ulcx_index_entry) * (size_t)indexTotal, hipMemcpyHostToDevice));
    if ((rc = index_ragged_any(who, e, d, di, dcnt, nullptr))) return rc;
    CKR(hipDeviceSynchronize());
    if (indexTotal) CKR(hipMemcpy(h_index, di, sizeof(ulcx_index_entry) * (size_t)indexTotal, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_nBlocks, dcnt, sizeof(int32_t) * (size_t)nFiles, hipMemcpyDeviceToHost));
    return ULCX_OK;
}

// ---- index while encoding (include/ulc_amd.h section 3): index_rows_any is the body of begin (slots == nullptr) and append.
// The decoder comes last among the checks: every other refusal needs no object (and so no device) to be seen.
static int index_rows_any(const char *who, ulcx_decoder *e, int nRows, bool append, const uint8_t *d_slots, int slotBytes, const int32_t *d_bits, int nBlocks,
                          ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, void *hipStream) {
    if (nRows < 1 || indexStride < 1 || !d_index || !d_nBlocks) return refuse(who, "bad argument (nRows %d, indexStride %d, or no index / counts)", nRows, indexStride);
    if (append && (!d_slots || !d_bits || slotBytes < 1 || nBlocks < 1)) return refuse(who, "bad argument (slotBytes %d, nBlocks %d, or no slots / sizes)", slotBytes, nBlocks);
    if (misaligned(who, "d_bits", d_bits, ULCX_ALIGN_WORD) || misaligned(who, "d_index", d_index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_nBlocks", d_nBlocks, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    // (one lane per block in a grid of 2^31 - 1 workgroups at the most: d_bits alone would be 512 GB)
    if (append && (long long)nRows * nBlocks > (0x7FFFFFFFLL << 6)) return refuse(who, "%d rows of %d blocks are more than one call takes", nRows, nBlocks);
    if ((long long)nRows * indexStride > (0x7FFFFFFFLL << 8)) return refuse(who, "%d rows of %d entries are more than one call takes", nRows, indexStride);
    if (!e) return refuse(who, "no decoder");
    CKR(hipSetDevice(e->device));
    if (!append) return ulcx_index_begin_launch(nRows, d_index, indexStride, d_nBlocks, (hipStream_t)hipStream);
    UlcxDecCtx c = e->ctx;
    c.in = d_slots; c.slot = slotBytes; c.inBytes = (long long)nRows * nBlocks * slotBytes;
    return ulcx_index_slots_launch(c, nRows, nBlocks, d_bits, d_index, indexStride, d_nBlocks, (hipStream_t)hipStream);
}
extern "C" int ulcx_index_begin_dev(ulcx_decoder *e, int nRows, ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, void *hipStream) {
    return index_rows_any("ulcx_index_begin_dev", e, nRows, false, nullptr, 0, nullptr, 0, d_index, indexStride, d_nBlocks, hipStream);
}
extern "C" int ulcx_index_slots_dev(ulcx_decoder *e, int nRows, const uint8_t *d_slots, int slotBytes, const int32_t *d_bits, int nBlocks,
                                    ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, void *hipStream) {
    return index_rows_any("ulcx_index_slots_dev", e, nRows, true, d_slots, slotBytes, d_bits, nBlocks, d_index, indexStride, d_nBlocks, hipStream);
}
extern "C" int ulcx_index_slots_host(ulcx_decoder *e, int nRows, const uint8_t *h_slots, int slotBytes, const int32_t *h_bits, int nBlocks,
                                     ulcx_index_entry *h_index, int indexStride, int32_t *h_nBlocks) {
    const char *who = "ulcx_index_slots_host";
    if (nRows < 1 || indexStride < 1 || !h_index || !h_nBlocks || !h_slots || !h_bits || slotBytes < 1 || nBlocks < 1) return refuse(who, "bad argument");
    for (int s = 0; s < nRows; s++)
        if (h_nBlocks[s] < 0 || h_nBlocks[s] > indexStride - 1) return refuse(who, "row %d counts %d blocks, outside 0 .. indexStride - 1 = %d", s, (int)h_nBlocks[s], indexStride - 1);
    if (!e) return refuse(who, "no decoder");
    CKR(hipSetDevice(e->device));
    const size_t NB = (size_t)nRows * nBlocks, nEnt = (size_t)nRows * (size_t)indexStride;
    DevTmp t; uint8_t *ds = nullptr; int32_t *db = nullptr, *dcnt = nullptr; ulcx_index_entry *di = nullptr;
    CKR(t.get(&ds, NB * (size_t)slotBytes)); CKR(t.get(&db, sizeof(int32_t) * NB));
    CKR(t.get(&dcnt, sizeof(int32_t) * nRows)); CKR(t.get(&di, sizeof(ulcx_index_entry) * nEnt));
    CKR(hipMemcpy(ds, h_slots, NB * (size_t)slotBytes, hipMemcpyHostToDevice));
    CKR(hipMemcpy(db, h_bits, sizeof(int32_t) * NB, hipMemcpyHostToDevice));
    CKR(hipMemcpy(dcnt, h_nBlocks, sizeof(int32_t) * nRows, hipMemcpyHostToDevice));
    CKR(hipMemcpy(di, h_index, sizeof(ulcx_index_entry) * nEnt, hipMemcpyHostToDevice));
    const int rc = index_rows_any(who, e, nRows, true, ds, slotBytes, db, nBlocks, di, indexStride, dcnt, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_index, di, sizeof(ulcx_index_entry) * nEnt, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(h_nBlocks, dcnt, sizeof(int32_t) * nRows, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
// ---- corpus splice (include/ulc_amd.h section 2): splice_any is the body of the two _dev forms, splice_host_any of the two host
// forms.  The decoder comes last among the checks, as in index_rows_any.
struct SpliceOut { uint8_t *payload; long long payloadStride; int32_t *payloadBytes, *maxBlock; ulcx_index_entry *index; int indexStride; int32_t *indexBlocks, *segStart; };
static bool ranges_meet(const void *a, unsigned long long na, const void *b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}
// the pointers and scalars both bodies check first, device or host pointers
static int splice_args_bad(const char *who, const UlcxCorpus &g, int nOut, const int32_t *segOffs, const ulcx_segment *seg, int nSeg, const SpliceOut &o) {
    if (corpus_null(g) || !segOffs || !seg || !o.payload || !o.payloadBytes || !o.index || !o.indexBlocks || !o.segStart) { refuse(who, "bad argument (a NULL pointer)"); return 1; }
    if (g.nFiles < 1 || nOut < 1 || nSeg < 1) { refuse(who, "bad argument (nFiles %d, nOut %d, nSeg %d)", g.nFiles, nOut, nSeg); return 1; }
    if (corpus_layout_bad(who, g)) return 1;
    if (o.payloadStride < 1 || o.indexStride < 2) { refuse(who, "bad argument (outPayloadStride %lld, outIndexStride %d: at least 1 and 2)", o.payloadStride, o.indexStride); return 1; }
    return 0;
}
static int splice_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int nOut, const int32_t *d_segOffs, const ulcx_segment *d_seg, int nSeg,
                      const SpliceOut &o, void *hipStream) {
    if (splice_args_bad(who, g, nOut, d_segOffs, d_seg, nSeg, o)) return ULCX_ERR_ARG;
    if (corpus_misaligned(who, g) || misaligned(who, "d_segOffs", d_segOffs, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_seg", d_seg, ULCX_ALIGN_WORD) || misaligned(who, "d_outPayloadBytes", o.payloadBytes, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_outMaxBlock", o.maxBlock, ULCX_ALIGN_WORD) || misaligned(who, "d_outIndex", o.index, ULCX_ALIGN_WORD) ||
        misaligned(who, "d_outIndexBlocks", o.indexBlocks, ULCX_ALIGN_WORD) || misaligned(who, "d_segStart", o.segStart, ULCX_ALIGN_WORD)) return ULCX_ERR_ARG;
    // (one lane per output block and per 16-byte line, each in a grid of 2^31 - 1 workgroups at the most; a payload range within 2^62)
    if ((long long)nOut * o.indexStride > (0x7FFFFFFFLL << 6) || o.payloadStride > (1LL << 40) || (long long)nOut * ((o.payloadStride + 30) / 16) > (0x7FFFFFFFLL << 8))
        return refuse(who, "%d output files of %d entries and %lld bytes are more than one call takes", nOut, o.indexStride, o.payloadStride);
    if (!g.ragged && g.payStride > (1LL << 40)) return refuse(who, "bad argument (payloadStride %lld)", g.payStride);
    const unsigned long long srcPay = (unsigned long long)g.payTotal, srcIdx = sizeof(ulcx_index_entry) * (unsigned long long)g.idxTotal;
    const unsigned long long outPay = (unsigned long long)nOut * (unsigned long long)o.payloadStride, outIdx = sizeof(ulcx_index_entry) * (unsigned long long)nOut * (unsigned long long)o.indexStride;
    if (ranges_meet(o.payload, outPay, g.pay, srcPay) || ranges_meet(o.payload, outPay, g.index, srcIdx) ||
        ranges_meet(o.index, outIdx, g.pay, srcPay) || ranges_meet(o.index, outIdx, g.index, srcIdx))
        return refuse(who, "the output payload or index overlaps the source's");
    if (!e) return refuse(who, "no decoder");
    CKR(hipSetDevice(e->device));
    UlcxDecCtx c = e->ctx;
    c.in = g.pay; c.inBytes = g.payTotal; c.packed = 1;
    UlcxSpliceArgs a = {};
    a.src = g;
    a.nOut = nOut; a.nSeg = nSeg; a.segOffs = d_segOffs; a.seg = d_seg; a.segStart = o.segStart;
    a.outPay = o.payload; a.outPayStride = o.payloadStride; a.outPayBytes = o.payloadBytes; a.outMaxBlock = o.maxBlock;
    a.outIndex = o.index; a.outIndexStride = o.indexStride; a.outIndexBlocks = o.indexBlocks;
    return ulcx_splice_launch(c, a, (hipStream_t)hipStream);
}
extern "C" int ulcx_corpus_splice_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                      const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                      int nOut, const int32_t *d_segOffs, const ulcx_segment *d_seg, int nSeg,
                                      uint8_t *d_outPayload, long long outPayloadStride, int32_t *d_outPayloadBytes, int32_t *d_outMaxBlock,
                                      ulcx_index_entry *d_outIndex, int outIndexStride, int32_t *d_outIndexBlocks, int32_t *d_segStart, void *hipStream) {
    const SpliceOut o = { d_outPayload, outPayloadStride, d_outPayloadBytes, d_outMaxBlock, d_outIndex, outIndexStride, d_outIndexBlocks, d_segStart };
    return splice_any("ulcx_corpus_splice_dev", e, ulcx_corpus_strided(nFiles, d_payload, payloadStride, d_payloadBytes, d_index, indexStride, d_indexBlocks),
                      nOut, d_segOffs, d_seg, nSeg, o, hipStream);
}
extern "C" int ulcx_corpus_splice_ragged_dev(ulcx_decoder *e, int nFiles, const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                             const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs, const int32_t *d_indexBlocks,
                                             int nOut, const int32_t *d_segOffs, const ulcx_segment *d_seg, int nSeg,
                                             uint8_t *d_outPayload, long long outPayloadStride, int32_t *d_outPayloadBytes, int32_t *d_outMaxBlock,
                                             ulcx_index_entry *d_outIndex, int outIndexStride, int32_t *d_outIndexBlocks, int32_t *d_segStart, void *hipStream) {
    const SpliceOut o = { d_outPayload, outPayloadStride, d_outPayloadBytes, d_outMaxBlock, d_outIndex, outIndexStride, d_outIndexBlocks, d_segStart };
    return splice_any("ulcx_corpus_splice_ragged_dev", e, ulcx_corpus_ragged(nFiles, d_payload, payloadTotal, d_payloadOffs, d_index, indexTotal, d_indexOffs, d_indexBlocks),
                      nOut, d_segOffs, d_seg, nSeg, o, hipStream);
}
// the host forms: the scalar checks of the _dev form first (on the host pointers), then what only a host form can refuse; the
// outputs go through device buffers of the call's own, and of the payload only the bytes the call wrote come back
static int splice_host_any(const char *who, ulcx_decoder *e, const UlcxCorpus &g, int nOut, const int32_t *h_segOffs, const ulcx_segment *h_seg, int nSeg,
                           const SpliceOut &o) {
    if (splice_args_bad(who, g, nOut, h_segOffs, h_seg, nSeg, o)) return ULCX_ERR_ARG;
    if (g.ragged && ragged_tables_bad(who, g)) return ULCX_ERR_ARG;
    if (h_segOffs[0] < 0 || h_segOffs[nOut] > nSeg) return refuse(who, "h_segOffs runs from %d to %d, outside 0 .. nSeg = %d", (int)h_segOffs[0], (int)h_segOffs[nOut], nSeg);
    for (int i = 0; i < nOut; i++)
        if (h_segOffs[i + 1] < h_segOffs[i]) return refuse(who, "h_segOffs falls from %d to %d at output file %d", (int)h_segOffs[i], (int)h_segOffs[i + 1], i);
    for (int j = 0; j < nSeg; j++) {
        const ulcx_segment &s = h_seg[j];
        if (s.File < 0 || s.File >= g.nFiles) return refuse(who, "segment %d names file %d of %d", j, (int)s.File, g.nFiles);
        if (s.First < 0 || s.Count < 0) return refuse(who, "segment %d is %d blocks from block %d", j, (int)s.Count, (int)s.First);
        if ((long long)s.First + s.Count > (long long)g.indexBlocks[s.File])
            return refuse(who, "segment %d ends at block %lld of a file of %d", j, (long long)s.First + s.Count, (int)g.indexBlocks[s.File]);
    }
    if (!e) return refuse(who, "no decoder");
    CKR(hipSetDevice(e->device));
    const size_t outEnt = (size_t)nOut * (size_t)o.indexStride;
    DevTmp t; UlcxCorpus d; uint8_t *dop = nullptr; int32_t *dso = nullptr, *dob = nullptr, *dom = nullptr, *docnt = nullptr, *dss = nullptr;
    ulcx_index_entry *doi = nullptr; ulcx_segment *dseg = nullptr;
    int rc = corpus_up(t, g, &d);
    if (rc) return rc;
    CKR(t.get(&dso, sizeof(int32_t) * ((size_t)nOut + 1))); CKR(t.get(&dseg, sizeof(ulcx_segment) * (size_t)nSeg)); CKR(t.get(&dss, sizeof(int32_t) * (size_t)nSeg));
    CKR(t.get(&dop, (size_t)nOut * (size_t)o.payloadStride)); CKR(t.get(&dob, sizeof(int32_t) * (size_t)nOut)); CKR(t.get(&dom, sizeof(int32_t) * (size_t)nOut));
    CKR(t.get(&docnt, sizeof(int32_t) * (size_t)nOut)); CKR(t.get(&doi, sizeof(ulcx_index_entry) * outEnt));
    CKR(hipMemcpy(dso, h_segOffs, sizeof(int32_t) * ((size_t)nOut + 1), hipMemcpyHostToDevice));
    CKR(hipMemcpy(dseg, h_seg, sizeof(ulcx_segment) * (size_t)nSeg, hipMemcpyHostToDevice));
    CKR(hipMemcpy(dss, o.segStart, sizeof(int32_t) * (size_t)nSeg, hipMemcpyHostToDevice));     // (segments of no output file go back as they came)
    const SpliceOut od = { dop, o.payloadStride, dob, dom, doi, o.indexStride, docnt, dss };
    if ((rc = splice_any(who, e, d, nOut, dso, dseg, nSeg, od, nullptr))) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(o.payloadBytes, dob, sizeof(int32_t) * (size_t)nOut, hipMemcpyDeviceToHost));
    if (o.maxBlock) CKR(hipMemcpy(o.maxBlock, dom, sizeof(int32_t) * (size_t)nOut, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(o.indexBlocks, docnt, sizeof(int32_t) * (size_t)nOut, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(o.index, doi, sizeof(ulcx_index_entry) * outEnt, hipMemcpyDeviceToHost));
    CKR(hipMemcpy(o.segStart, dss, sizeof(int32_t) * (size_t)nSeg, hipMemcpyDeviceToHost));
    for (int i = 0; i < nOut; i++)
        if (o.payloadBytes[i] > 0)
            CKR(hipMemcpy(o.payload + (size_t)i * (size_t)o.payloadStride, dop + (size_t)i * (size_t)o.payloadStride, (size_t)o.payloadBytes[i], hipMemcpyDeviceToHost));
    return ULCX_OK;
}
extern "C" int ulcx_corpus_splice_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                       const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                       int nOut, const int32_t *h_segOffs, const ulcx_segment *h_seg, int nSeg,
                                       uint8_t *h_outPayload, long long outPayloadStride, int32_t *h_outPayloadBytes, int32_t *h_outMaxBlock,
                                       ulcx_index_entry *h_outIndex, int outIndexStride, int32_t *h_outIndexBlocks, int32_t *h_segStart) {
    const SpliceOut o = { h_outPayload, outPayloadStride, h_outPayloadBytes, h_outMaxBlock, h_outIndex, outIndexStride, h_outIndexBlocks, h_segStart };
    return splice_host_any("ulcx_corpus_splice_host", e, ulcx_corpus_strided(nFiles, h_payload, payloadStride, h_payloadBytes, h_index, indexStride, h_indexBlocks),
                           nOut, h_segOffs, h_seg, nSeg, o);
}
extern "C" int ulcx_corpus_splice_ragged_host(ulcx_decoder *e, int nFiles, const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                              const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs, const int32_t *h_indexBlocks,
                                              int nOut, const int32_t *h_segOffs, const ulcx_segment *h_seg, int nSeg,
                                              uint8_t *h_outPayload, long long outPayloadStride, int32_t *h_outPayloadBytes, int32_t *h_outMaxBlock,
                                              ulcx_index_entry *h_outIndex, int outIndexStride, int32_t *h_outIndexBlocks, int32_t *h_segStart) {
    const SpliceOut o = { h_outPayload, outPayloadStride, h_outPayloadBytes, h_outMaxBlock, h_outIndex, outIndexStride, h_outIndexBlocks, h_segStart };
    return splice_host_any("ulcx_corpus_splice_ragged_host", e, ulcx_corpus_ragged(nFiles, h_payload, payloadTotal, h_payloadOffs, h_index, indexTotal, h_indexOffs, h_indexBlocks),
                           nOut, h_segOffs, h_seg, nSeg, o);
}
extern "C" int ulcx_index_check(const ulcx_index_entry *row, int nBlocks, int indexStride, long long payloadBytes) {
    const char *who = "ulcx_index_check";
    if (!row) return refuse(who, "no index");
    if (nBlocks < 0 || nBlocks >= indexStride) return refuse(who, "%d blocks in a row of %d entries", nBlocks, indexStride);
    if (row[0].ByteOffs != 0 || row[0].RngState != 1234567u) return refuse(who, "entry 0 is {%d, %u}, not {0, 1234567}", (int)row[0].ByteOffs, (unsigned)row[0].RngState);
    for (int k = 1; k <= nBlocks; k++)
        if (row[k].ByteOffs <= row[k - 1].ByteOffs) return refuse(who, "entry %d starts at byte %d, entry %d at %d", k, (int)row[k].ByteOffs, k - 1, (int)row[k - 1].ByteOffs);
    if ((long long)row[nBlocks].ByteOffs > payloadBytes) return refuse(who, "the index closes at byte %d of a payload of %lld", (int)row[nBlocks].ByteOffs, payloadBytes);
    return ULCX_OK;
}
extern "C" int ulcx_decoder_set_resident_index(ulcx_decoder *e, const ulcx_index_entry *h_index, int indexStride, const int32_t *h_nBlocks) {
    const char *who = "ulcx_decoder_set_resident_index";
    if (!e || !h_index || !h_nBlocks || indexStride < 1) return refuse(who, "bad argument");
    if (!e->d_pay) return refuse(who, "no payload uploaded");
    CKR(hipSetDevice(e->device));
    std::vector<int32_t> payBytes((size_t)e->B);
    CKR(hipMemcpy(payBytes.data(), e->d_payBytes, sizeof(int32_t) * e->B, hipMemcpyDeviceToHost));
    for (int s = 0; s < e->B; s++) {
        const long long avail = std::min<long long>(payBytes[(size_t)s], e->payStride);
        if (ulcx_index_check(h_index + (size_t)s * indexStride, h_nBlocks[s], indexStride, avail)) {
            const std::string why = ulcx_last_error();
            return refuse(who, "stream %d: %s", s, why.c_str());
        }
    }
    // checked: from here on the index the decoder had is replaced
    e->idxStride = 0;
    const size_t nEnt = (size_t)e->B * (size_t)indexStride;
    int rc = dregrow(e->allocs, &e->d_index, nEnt, false);
    if (!rc && !e->d_idxBlocks) rc = dalloc(e->allocs, &e->d_idxBlocks, (size_t)e->B, false);
    if (rc) return rc;
    CKR(hipMemcpy(e->d_index, h_index, sizeof(ulcx_index_entry) * nEnt, hipMemcpyHostToDevice));
    CKR(hipMemcpy(e->d_idxBlocks, h_nBlocks, sizeof(int32_t) * e->B, hipMemcpyHostToDevice));
    e->idxStride = indexStride;
    return ULCX_OK;
}

// ---------------------------------------------------------------------------
// Stream slots (include/ulc_amd.h): per-stream reset, save / load.  The copies are ulcx_slots.hip's; what they work on comes
// from the slot_* overloads of the object's type.  (The subset calls are with their families above.)
// ---------------------------------------------------------------------------
template <class OBJ> static int slots_reset_dev(const char *who, OBJ *e, const int32_t *d_slots, int n, void *hipStream) {
    if (!e) return refuse(who, "no object");
    if (slots_list_bad(who, d_slots, n, e->B)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    slot_touch(e);
    return ulcx_slots_reset(slot_obj_rows(e), d_slots, n, slot_geom(e, false), (hipStream_t)hipStream);
}
template <class OBJ> static int slots_save_dev(const char *who, OBJ *e, const int32_t *d_slots, int n, uint8_t *d_state, void *hipStream) {
    if (!e || !d_state) return refuse(who, "bad argument");
    if (slots_list_bad(who, d_slots, n, e->B) || misaligned(who, "d_state", d_state, ULCX_ALIGN_STATE)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    return ulcx_slots_gather(slot_obj_rows(e), slot_record_rows(e, d_state), d_slots, n, slot_geom(e, true), (hipStream_t)hipStream);
}
template <class OBJ> static int slots_load_dev(const char *who, OBJ *e, const int32_t *d_slots, int n, const uint8_t *d_state, void *hipStream) {
    if (!e || !d_state) return refuse(who, "bad argument");
    if (slots_list_bad(who, d_slots, n, e->B) || misaligned(who, "d_state", d_state, ULCX_ALIGN_STATE)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    slot_touch(e);
    return ulcx_slots_scatter(slot_obj_rows(e), slot_record_rows(e, (uint8_t *)d_state), d_slots, n, slot_geom(e, true), (hipStream_t)hipStream);
}
// host forms: the checked list to the device, the _dev form on the null stream, one synchronisation; save / load: the records
// through a device buffer of the call's own
template <class OBJ> static int slots_reset_host(const char *who, OBJ *e, const int32_t *h_slots, int n) {
    if (!e) return refuse(who, "no object");
    if (slots_host_bad(who, h_slots, n, e->B)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    int rc = slots_list_up(e, h_slots, n);
    if (!rc) rc = slots_reset_dev(who, e, e->subSlots, n, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    return ULCX_OK;
}
template <class OBJ> static int slots_save_host(const char *who, OBJ *e, const int32_t *h_slots, int n, uint8_t *h_state) {
    if (!e || !h_state) return refuse(who, "bad argument");
    if (slots_host_bad(who, h_slots, n, e->B)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t bytes = (size_t)n * slot_state_bytes(e);
    DevTmp t; uint8_t *ds = nullptr;
    CKR(t.get(&ds, bytes));
    int rc = slots_list_up(e, h_slots, n);
    if (!rc) rc = slots_save_dev(who, e, e->subSlots, n, ds, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    CKR(hipMemcpy(h_state, ds, bytes, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
template <class OBJ> static int slots_load_host(const char *who, OBJ *e, const int32_t *h_slots, int n, const uint8_t *h_state) {
    if (!e || !h_state) return refuse(who, "bad argument");
    if (slots_host_bad(who, h_slots, n, e->B)) return ULCX_ERR_ARG;
    if (record_headers_bad(who, h_state, n, slot_state_bytes(e), slot_geom(e, true).header)) return ULCX_ERR_ARG;
    CKR(hipSetDevice(e->device));
    const size_t bytes = (size_t)n * slot_state_bytes(e);
    DevTmp t; uint8_t *ds = nullptr;
    CKR(t.get(&ds, bytes));
    CKR(hipMemcpy(ds, h_state, bytes, hipMemcpyHostToDevice));
    int rc = slots_list_up(e, h_slots, n);
    if (!rc) rc = slots_load_dev(who, e, e->subSlots, n, ds, nullptr);
    if (rc) return rc;
    CKR(hipDeviceSynchronize());
    return ULCX_OK;
}
extern "C" int ulcx_encoder_reset_streams_dev(ulcx_encoder *e, const int32_t *d_slots, int n, void *st) { return slots_reset_dev("ulcx_encoder_reset_streams_dev", e, d_slots, n, st); }
extern "C" int ulcx_encoder_save_streams_dev(ulcx_encoder *e, const int32_t *d_slots, int n, uint8_t *d_state, void *st) { return slots_save_dev("ulcx_encoder_save_streams_dev", e, d_slots, n, d_state, st); }
extern "C" int ulcx_encoder_load_streams_dev(ulcx_encoder *e, const int32_t *d_slots, int n, const uint8_t *d_state, void *st) { return slots_load_dev("ulcx_encoder_load_streams_dev", e, d_slots, n, d_state, st); }
extern "C" int ulcx_decoder_reset_streams_dev(ulcx_decoder *e, const int32_t *d_slots, int n, void *st) { return slots_reset_dev("ulcx_decoder_reset_streams_dev", e, d_slots, n, st); }
extern "C" int ulcx_decoder_save_streams_dev(ulcx_decoder *e, const int32_t *d_slots, int n, uint8_t *d_state, void *st) { return slots_save_dev("ulcx_decoder_save_streams_dev", e, d_slots, n, d_state, st); }
extern "C" int ulcx_decoder_load_streams_dev(ulcx_decoder *e, const int32_t *d_slots, int n, const uint8_t *d_state, void *st) { return slots_load_dev("ulcx_decoder_load_streams_dev", e, d_slots, n, d_state, st); }
extern "C" int ulcx_encoder_reset_streams_host(ulcx_encoder *e, const int32_t *h_slots, int n) { return slots_reset_host("ulcx_encoder_reset_streams_host", e, h_slots, n); }
extern "C" int ulcx_encoder_save_streams_host(ulcx_encoder *e, const int32_t *h_slots, int n, uint8_t *h_state) { return slots_save_host("ulcx_encoder_save_streams_host", e, h_slots, n, h_state); }
extern "C" int ulcx_encoder_load_streams_host(ulcx_encoder *e, const int32_t *h_slots, int n, const uint8_t *h_state) { return slots_load_host("ulcx_encoder_load_streams_host", e, h_slots, n, h_state); }
extern "C" int ulcx_decoder_reset_streams_host(ulcx_decoder *e, const int32_t *h_slots, int n) { return slots_reset_host("ulcx_decoder_reset_streams_host", e, h_slots, n); }
extern "C" int ulcx_decoder_save_streams_host(ulcx_decoder *e, const int32_t *h_slots, int n, uint8_t *h_state) { return slots_save_host("ulcx_decoder_save_streams_host", e, h_slots, n, h_state); }
extern "C" int ulcx_decoder_load_streams_host(ulcx_decoder *e, const int32_t *h_slots, int n, const uint8_t *h_state) { return slots_load_host("ulcx_decoder_load_streams_host", e, h_slots, n, h_state); }

// diagnostic, only in a `make EXTRA=-DULCX_DSYN_STAMPS` build (tools/dsyn_stamps.py): first nBytes of the general-path staging
// buffer, where that build leaves per-phase cycle counts
#ifdef ULCX_DSYN_STAMPS
extern "C" int ulcx_decoder_debug_scratch(ulcx_decoder *e, void *h_out, size_t strideBytes, size_t nBytes, int nStreams);
extern "C" int ulcx_decoder_debug_scratch(ulcx_decoder *e, void *h_out, size_t strideBytes, size_t nBytes, int nStreams) {
    if (!e || !h_out) return refuse("ulcx_decoder_debug_scratch", "bad argument");
    CKR(hipSetDevice(e->device));
    CKR(hipDeviceSynchronize());
    for (int s = 0; s < nStreams && s < e->B; s++)
        CKR(hipMemcpy((char *)h_out + (size_t)s * nBytes, (const char *)e->ctx.scratch + (size_t)s * strideBytes, nBytes, hipMemcpyDeviceToHost));
    return ULCX_OK;
}
#endif
// per-stage hipEvents around every kernel (ulcx_*_stage_ms): on by default; a caller that does not read them can switch
// them off - each record is a marker packet in the stream between two kernels
extern "C" int ulcx_encoder_set_timing(ulcx_encoder *e, int on) { if (!e) return refuse("ulcx_encoder_set_timing", "no encoder"); e->timing = on != 0; if (!on) e->evRecorded = false; return ULCX_OK; }
extern "C" int ulcx_decoder_set_timing(ulcx_decoder *e, int on) { if (!e) return refuse("ulcx_decoder_set_timing", "no decoder"); e->timing = on != 0; if (!on) e->evRecorded = false; return ULCX_OK; }
static const char *kDecStage[ULCX_DEC_STAGES] = { "k_dscan", "k_dsyn" };
extern "C" const char *ulcx_decoder_stage_name(int i) { return (i >= 0 && i < ULCX_DEC_STAGES) ? kDecStage[i] : ""; }
extern "C" int ulcx_decoder_stage_ms(ulcx_decoder *e, float *ms, int maxStages) {
    if (!e || !e->evRecorded) return 0;
    int n = 0;
    for (int i = 0; i < ULCX_DEC_STAGES && i < maxStages; i++) {
        float t = 0;
        if (hipEventElapsedTime(&t, e->ev[i], e->ev[i + 1]) != hipSuccess) break;
        ms[n++] = t;
    }
    return n;
}
