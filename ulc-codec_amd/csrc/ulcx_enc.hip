// ulcx_enc.hip — batched ulc-codec encoder for gfx950 (MI355X), hand-written HIP.
//
// One call encodes K consecutive blocks of B independent streams.  Pipeline
// (reference call stack SURVEY.md §3A):
//   wc_energy / wc_forward / wc_backward / wc_integrate / wc_decide
//        transient detector -> WindowCtrl per block   (ulcEncoder_WindowControl.c:41-239)
//   xf   one workgroup per block: frames from the input timeline (closed form of the
//        lapping FIFO, BlockTransform.c:175-224), sine window, MDCT+MDST through two
//        DCT-IV = complex FFTs staged entirely in LDS, normalise, keys, per-line
//        energies                                      (BlockTransform.c:229-281)
//   cplx        ordered f32 sums -> BlockComplexity, nOutCoef (BlockTransform.c:279-325, ulcEncoder.c:140-158)
//   bark_uniform/bark_levels/nbark/nline  noise log-spectrum (un-decimated blocks on the geometry-uniform
//               kernel, the rest lane per subblock)    (ulcEncoder_Psyopt.c:168-250)
//   pbark       masking Bark levels                    (ulcEncoder_Psyopt.c:60-155)
//   select      one wave per block: keys (coefficient + masking level, BlockTransform.c:337-345) in registers,
//               the nOutCoef-th largest by bisection; exact heapsort emulation only for tie groups
//               straddling the cut                     (BlockTransform.c:20-77)
//   encode/pack nybble stream                          (ulcEncoder_Encode.c:23-360, ulcEncoder_NoiseFill.c)
// All float arithmetic is written in the reference's operation order and this file is
// compiled with -ffp-contract=off: no fused multiply-add is formed anywhere except the
// explicit ones inside the glibc restatements (ulcx_libm.h).
#include "ulcx_enc_dev.h"

// ---------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------
// 4 padded arrays of BS/2 complex + BS/4 twiddles + 32 bytes (once the non-zero counter's: xf_block's offsets keep the slot)
// (+ BS/2 floats of line energies for C > 2)
static size_t ulcx_enc_xf_lds_bytes(int BS, int C) {
    if (BS > 8192) return (size_t)BS * 4;                       // k_xf_big: one unpadded array of BS/2 complex
    int ps = ulcx_xf_pad_shift(BS, C);
    size_t z = (size_t)4 * (BS + (BS >> ps)) * 4;               // four padded arrays of BS/2 complex
    size_t full = z + (size_t)BS * 2 + 32 + (C > 2 ? (size_t)BS * 2 : 0);
    return full <= ULCX_LDS_LIMIT ? full : z + (size_t)BS * 2 + 32;   // (C > 2 at BlockSize 8192: twiddles stay in global memory)
}

// the analysis call's transform: the two MDCT arrays + BS/4 twiddles (+ the counter's slot, unused)
static size_t ulcx_enc_xfa_lds_bytes(int BS, int C) {
    if (BS > 8192) return (size_t)BS * 4;                       // k_xfa_big: as k_xf_big
    int ps = ulcx_xf_pad_shift(BS, C);
    return (size_t)2 * (BS + (BS >> ps)) * 4 + (size_t)BS * 2 + 32;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ulcx_set_error("%s: %s", #x, hipGetErrorString(e_)); return ULCX_ERR_HIP; } } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// One pick per kernel family: the instantiation for the call's sample type (float | PCM16), geometry and pass is chosen in
// one function; raising its dynamic-LDS limit and launching it both use what that function returns.
typedef void (*RangeKernel)(UlcxEncCtx, int, int);            // blocks [k0, k1) of every stream
typedef void (*PassKernel)(UlcxEncCtx, int);                  // (finalPass)
typedef void (*CallKernel)(UlcxEncCtx);

static RangeKernel wc_energy_fn(const UlcxEncCtx &c) { return c.pcm16 ? k_wc_energy<int16_t> : k_wc_energy<float>; }
static RangeKernel wc_ef_fn(const UlcxEncCtx &c) { return c.pcm16 ? k_wc_ef<EF_NW, int16_t> : k_wc_ef<EF_NW, float>; }
static CallKernel state_update_fn(const UlcxEncCtx &c) { return c.pcm16 ? k_state_update<int16_t> : k_state_update<float>; }

// the transform: the encode call's or the analysis call's MDCT-only one; above BlockSize 8192 one array at a time (*_big)
template <typename IN> static RangeKernel xf_fn_in(const UlcxEncCtx &c, bool mdctOnly) {
    if (c.BS > 8192) return mdctOnly ? k_xfa_big<IN> : k_xf_big<IN>;
    if (c.C == 2) return mdctOnly ? k_xfa<true, IN> : k_xf<true, IN>;
    return mdctOnly ? k_xfa<false, IN> : k_xf<false, IN>;
}
static RangeKernel xf_fn(const UlcxEncCtx &c, bool mdctOnly) { return c.pcm16 ? xf_fn_in<int16_t>(c, mdctOnly) : xf_fn_in<float>(c, mdctOnly); }

// The selection with one wave per block (pair: stereo BlockSize 4096, a wave per channel) for R = C * BlockSize / 64 keys per
// lane; NULL: a geometry only the generic k_select covers.  rates: the per-stream-rates counterparts, which leave the blocks of
// the other kind.  pass: 0 = one-pass call, 1 = first probe of a rate search (stores the ordered keys), 2 = later ones.
template <int PASS> static PassKernel select_fn_pass(const UlcxEncCtx &c, bool pair, bool rates) {
#define SEL(R, L) (rates ? (PassKernel)k_select_wave_rates<R, L, PASS> : (PassKernel)k_select_wave<R, L, PASS>)
    switch (c.C * c.BS / 64) {
        case 128:                                            // (one wave: ~200 VGPRs, two waves per SIMD)
            if (pair) return rates ? k_select_pair_rates<64, 12, PASS> : k_select_pair<64, 12, PASS>;
            return SEL(128, 0);
        case 64: return c.lgBS == 11 ? SEL(64, 11) : SEL(64, 0);       // (11: stereo BlockSize 2048; with a wave per channel its
                                                                       //  selection is 1.08 -> 1.23 ms: barriers)
        case 32: return SEL(32, 0);
        case 16: return SEL(16, 0);
        case 8:  return SEL(8, 0);
        case 4:  return SEL(4, 0);
        default: return nullptr;
    }
#undef SEL
}
static PassKernel select_fn(const UlcxEncCtx &c, bool pair, bool rates, int pass) {
    return pass == 1 ? select_fn_pass<1>(c, pair, rates) : pass == 2 ? select_fn_pass<2>(c, pair, rates) : select_fn_pass<0>(c, pair, rates);
}

// A launch with more than 48 KiB of dynamic LDS: raise the kernel's limit to this launch's size.  Per launch, not per
// encoder: the attribute belongs to the function on the device, and encoders of different geometry share it.
static int allow_lds(const void *fn, size_t lds) {
    if (lds > 48 * 1024) CK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return ULCX_OK;
}

static void launch_wc_energy(const UlcxEncCtx &c, unsigned grid, hipStream_t st, int k0, int k1) {
    hipLaunchKernelGGL(wc_energy_fn(c), dim3(grid), dim3(WG), 0, st, c, k0, k1);
}

static void launch_wc_ef(const UlcxEncCtx &c, hipStream_t st, int k0, int k1) {
    static_assert(EF_LDS_BYTES <= 48 * 1024, "k_wc_ef: raise the dynamic LDS limit with hipFuncSetAttribute");
    hipLaunchKernelGGL(wc_ef_fn(c), dim3((c.B + EF_SPW - 1) / EF_SPW), dim3(EF_NW * 64), EF_LDS_BYTES, st, c, k0, k1);
}

static void launch_state_update(const UlcxEncCtx &c, hipStream_t st) {
    hipLaunchKernelGGL(state_update_fn(c), dim3(c.B), dim3(WG), 0, st, c);
}

// Per-kernel hipEvents (on the launch stream) bracket every kernel of the first pass so
// bench.py can price each one against the roofline live; ev holds ULCX_ENC_STAGES+1 events.
const char *const ulcx_enc_stage_names[ULCX_ENC_STAGES_REPORTED] = {
    "k_wc_energy", "k_wc_forward", "k_wc_backward", "k_wc_integrate", "k_wc_decide",
    "k_xf", "k_cplx", "k_pbark", "k_mask",
    "k_select", "k_nbark", "(k_nline: gone)", "k_heapsel", "k_nsums", "k_tails", "k_encode_wave", "k_encode_units", "k_pack", "cbr_probe_passes", "k_state_update", "wc_pipeline_exposed",
};

struct StageMarks { hipEvent_t *ev; int stage; };             // ev NULL (timing off, or a pass that is not the first): MARK does nothing
#define MARK(mk, s) do { if ((mk).ev) CK(hipEventRecord((mk).ev[(mk).stage++], s)); } while (0)

// The front half of a call: the window-control pipeline beside the transform chunks and the chunks' ordered sums.
// what: the encode call's kernels (k_xf, k_cplx), the analysis call's (k_xfa, k_cplxa), the analysis call on the encode
// call's transform (k_xf, k_cplxa: the plain launch subset, for timing comparisons) or window control alone with k_cplxa
// behind it to write the window codes out (an analysis call that asks for nothing else).
enum { ULCX_FRONT_ENCODE = 0, ULCX_FRONT_ANALYSE = 1, ULCX_FRONT_ANALYSE_KXF = 2, ULCX_FRONT_WC_ONLY = 3 };
static int launch_front(const UlcxEncCtx &c, hipStream_t st, StageMarks &mk, const UlcxEncAux &aux, const int what) {
    UlcxEncSync &sy = aux.sync;
    hipStream_t side = sy.side, side2 = sy.side2, side3 = sy.side3;
    const int SG = (c.B + 63) / 64;
    // Chunks of blocks: the window-control kernels of chunk j+1.. (two stream-long serial recurrences, a few
    // hundred waves: latency-bound, nearly no machine resources) run on the side stream beside the
    // transform of chunk j on the main stream.  wcPipe = 1 keeps everything on the main stream.
    const int nCh = aux.wcPipe;
    const bool mdctOnly = (what == ULCX_FRONT_ANALYSE);
    const RangeKernel xf = (what == ULCX_FRONT_WC_ONLY) ? nullptr : xf_fn(c, mdctOnly);
    const size_t lds = mdctOnly ? ulcx_enc_xfa_lds_bytes(c.BS, c.C) : ulcx_enc_xf_lds_bytes(c.BS, c.C);
    if (xf) TRY(allow_lds((const void *)xf, lds));
    auto transform = [&](int k0, int k1) {
        if (xf) hipLaunchKernelGGL(xf, dim3((unsigned)((c.B * (k1 - k0) + 7) / 8) * 8), dim3(WG), lds, st, c, k0, k1);
    };
    const bool wcFuse = c.C == 2 && aux.wcFuse;   // stereo: k_wc_energy + k_wc_forward in one kernel (k_wc_ef)
    aux.nXf = 0;
    if (nCh <= 1) {
        if (wcFuse) { MARK(mk, st); launch_wc_ef(c, st, 0, c.K);                                                  MARK(mk, st); }
        else {
        launch_wc_energy(c, (unsigned)(SG * ((c.K * c.BS) / 64)), st, 0, c.K);                                    MARK(mk, st);
        hipLaunchKernelGGL(k_wc_forward, dim3((c.B * 2 + 63) / 64), dim3(64), 0, st, c, 0, c.K);                  MARK(mk, st);
        }
        hipLaunchKernelGGL(k_wc_backward, dim3(SG * c.K), dim3(64), 0, st, c, 0, c.K);                            MARK(mk, st);
        hipLaunchKernelGGL(k_wc_integrate, dim3((c.B + 63) / 64), dim3(64), 0, st, c, 0, c.K);                    MARK(mk, st);
        hipLaunchKernelGGL(k_wc_decide, dim3((c.B * c.K + 63) / 64), dim3(64), 0, st, c, 0, c.K);                 MARK(mk, st);
        transform(0, c.K);
        MARK(mk, st);
        return ULCX_OK;
    }
    for (int i = 0; i < 5; i++) MARK(mk, st);              // (window-control stages: hidden in the k_xf interval in this mode)
    // side: envelope + forward recurrence of step w (the sample-rate chain, back to back over the steps);
    // side2: backward_w behind forward_w;  side3: integrate_w, decide_w behind backward_w;
    // main: transform chunk j behind the step that decides its last block.  The first chunk is a single block so the transform starts early.
    // The steps and the cuts: ulcx_front_plan (ulcx_internal.h), which ulcx_encoder_debug_front_plan reports too.
    const UlcxFrontPlan fp = ulcx_front_plan(c.K, nCh, aux.wcSteps);
    const int nW = fp.nW;
    const int *cut = fp.cut, *wcs = fp.wcs;
    CK(hipEventRecord(sy.wcStart, st));
    CK(hipStreamWaitEvent(side, sy.wcStart, 0));
    int jx = 0;                                        // next transform chunk to enqueue
    for (int w = 0; w < nW; w++) {
        const int k0 = wcs[w], k1 = wcs[w + 1], kc = k1 - k0;
        if (wcFuse) launch_wc_ef(c, side, k0, k1);
        else {
            launch_wc_energy(c, (unsigned)(SG * ((kc * c.BS) / 64)), side, k0, k1);
            hipLaunchKernelGGL(k_wc_forward, dim3((c.B * 2 + 63) / 64), dim3(64), 0, side, c, k0, k1);
        }
        CK(hipEventRecord(sy.wcForward[w], side));
        CK(hipStreamWaitEvent(side2, sy.wcForward[w], 0));
        hipLaunchKernelGGL(k_wc_backward, dim3(SG * kc), dim3(64), 0, side2, c, k0, k1);
        CK(hipEventRecord(sy.wcBackward[w], side2));
        CK(hipStreamWaitEvent(side3, sy.wcBackward[w], 0));
        hipLaunchKernelGGL(k_wc_integrate, dim3((c.B + 63) / 64), dim3(64), 0, side3, c, k0, k1);
        hipLaunchKernelGGL(k_wc_decide, dim3((c.B * kc + 63) / 64), dim3(64), 0, side3, c, k0, k1);
        CK(hipEventRecord(sy.wcDecided[w], side3));
        // transform chunks whose last block is now decided
        while (jx < nCh && cut[jx + 1] <= k1) {
            CK(hipStreamWaitEvent(st, sy.wcDecided[w], 0));
            if (mk.ev) CK(hipEventRecord(sy.xfTiming[2 * jx], st));
            if (!(ULCX_DBG(c) & 0x2000))               // (ablation build: window control alone)
            transform(cut[jx], cut[jx + 1]);
            if (mk.ev) CK(hipEventRecord(sy.xfTiming[2 * jx + 1], st));
            CK(hipEventRecord(sy.xfChunkDone[jx], st));
            jx++;
        }
    }
    aux.nXf = nCh;
    MARK(mk, st);
    // the ordered complexity sums (k_cplx: lane-serial, HBM-bound) per transform chunk, on the envelope kernels' stream
    // (all of those are enqueued by now): only the last chunk's are left beside the masking sums
    for (int j = 0; j < nCh; j++) {
        CK(hipStreamWaitEvent(side, sy.xfChunkDone[j], 0));
        const int kc2 = cut[j + 1] - cut[j];
        if (what == ULCX_FRONT_ENCODE) hipLaunchKernelGGL(k_cplx, dim3((c.B * kc2 + 63) / 64), dim3(64), 0, side, c, cut[j], cut[j + 1]);
        else hipLaunchKernelGGL(k_cplxa, dim3((c.B * kc2 + 63) / 64), dim3(64), 0, side, c, cut[j], cut[j + 1]);
    }
    CK(hipEventRecord(sy.cplxChunksDone, side));
    return ULCX_OK;
}

// What a call's back half launches with: host arithmetic over the geometry, done once.
struct EncPlan {
    int NB, N, nUnits;                   // blocks of the call, coefficients per block, (block, channel, subblock) units
    bool aside;                          // side streams: noise chain, k_cplx, k_tails, k_state_update and the exact path leave the main stream
    int probes;                          // rate-search passes in front of the final one (0: one-pass call)
    size_t barkLds;                      // k_bark_uniform
    bool selWave, selPair;               // the selection: one wave per block (else the generic k_select) / a wave per channel
    size_t selLds;                       // ... and its LDS per workgroup
    int ldsEntries, fbGrid; size_t heapLds;      // exact path's heapsort
    WaveCaps capS, capM, capF;           // wave-writer capacities: small, medium (retries of probes and of the exact path), full
    bool haveFull, haveMid;
    int nsSlots;
};
static int enc_probes(const UlcxEncCtx &c, int N) {         // (see EncPlan::probes below)
    int n = 0;
    if (c.mode != ULCX_MODE_VBR || c.rates != nullptr) { n = 2; for (int m = N; m > 1; m >>= 1) n++; }
    return n;
}
static EncPlan enc_plan(const UlcxEncCtx &c, const UlcxEncAux &aux) {
    EncPlan p;
    p.NB = c.B * c.K; p.N = c.C * c.BS; p.nUnits = p.NB * c.C * 4;
    p.aside = aux.sync.side != nullptr;
    // VBR: one pass.  CBR/ABR: the reference's binary search (ulcEncoder.c:98-110) needs at most
    // ceil(log2(MaxCoef))+1 probes; every block runs its own search in lock step, then one final pass.
    // Per-stream rates (c.rates): the host does not know the table, so such a call runs the rate search's launch sequence
    // whatever it holds (VBR blocks skip every probe on the device).
    // No read-back: the host always enqueues the full count and a pass whose blocks have all converged (c.cbrLive,
    // counted down on the device) returns at the top of every kernel - nothing inside the call waits for the device.
    p.probes = enc_probes(c, p.N);
    p.barkLds = (size_t)c.barkRing * 3 * 64 * 8 + (size_t)2 * BK_TILE_FLOATS * 4;
    const int R = p.N / 64;
    p.selWave = (R == 4 || R == 8 || R == 16 || R == 32 || R == 64 || R == 128);
    p.selPair = (R == 128 && c.C == 2 && c.selPair);                                   // stereo BlockSize 4096
    p.selLds = (size_t)(p.selPair ? 1 : 4) * ulcx_sel_lds_words(c.BS) * sizeof(float);      // (mono BlockSize 8192: 67 KB)
    p.ldsEntries = ((size_t)p.N * 8 <= ULCX_HEAP_LDS_BYTES) ? p.N : 0;
    p.heapLds = p.ldsEntries ? (size_t)p.N * 8 + (size_t)p.N / 8 : 0;
    p.fbGrid = p.NB < ULCX_HEAP_GRID ? p.NB : ULCX_HEAP_GRID;
    // wave-kernel capacities: small (ordinary blocks, high occupancy) and full (any unit of this block size)
    p.capS = { WAVE_SK, WAVE_SZ, WAVE_SN };
    p.capF = { (c.BS + 63) & ~63, ((c.BS / 2) + 63) & ~63, 4 * c.BS + 64 };
    while ((size_t)wavecaps_lds(p.capF) * 4 > 150 * 1024) {     // largest that 4 waves fit in LDS; beyond it k_encode_units
        p.capF.k = (p.capF.k / 2 + 63) & ~63; p.capF.z = (p.capF.z / 2 + 63) & ~63; p.capF.nyb = p.capF.nyb / 2 + 32;
    }
    p.haveFull = p.capF.k > p.capS.k;
    // rate-control probes: k_cplx has already taken every probe that is over budget for certain, so a probe keeps at most
    // ~BitBudget/4 coefficients per block: the retry of the small launch runs with medium capacities (2 workgroups per CU
    // instead of 1), and what even they cannot hold goes to k_encode_units
    p.capM = { 1024, 512, 4096 };
    p.haveMid = p.capM.k < p.capF.k;
    p.nsSlots = aux.nsSlots;
    return p;
}

// the noise log-spectrum (k_nbark: lane-serial ordered sums, latency-bound); un-decimated blocks on the geometry-uniform kernel
static void launch_noise(const UlcxEncCtx &c, const EncPlan &p, hipStream_t s2) {
    if (c.barkRing) {
        hipLaunchKernelGGL(k_bark_uniform<true>, dim3((p.NB * c.C + 63) / 64), dim3(256), p.barkLds, s2, c);
        hipLaunchKernelGGL(k_bark_levels<true>, dim3((unsigned)(((size_t)p.NB * c.C * 32 + WG - 1) / WG)), dim3(WG), 0, s2, c);
    }
    hipLaunchKernelGGL(k_nbark, dim3((p.nUnits + 63) / 64), dim3(64), 0, s2, c, c.barkRing ? 1 : 0);
}

// Behind the transform: the ordered sums (k_cplx), the masking Bark levels on the main stream and, with side streams, the
// noise log-spectrum and the state for the next call beside them.
// Three lane-serial latency-bound kernels (k_pbark, k_cplx, k_nbark) fill the machine's wave slots by themselves; k_cplx
// (~1000 waves; per transform chunk in a pipelined call: launch_front) runs beside k_pbark, the noise chain (it depends on
// the transform only) beside the masking sums and the throughput-bound selection.
static int launch_psy(const UlcxEncCtx &c, const EncPlan &p, UlcxEncSync &sy, hipStream_t st, StageMarks &mk, bool cplxChunked) {
    if (c.barkRing) { TRY(allow_lds((const void *)k_bark_uniform<true>, p.barkLds)); TRY(allow_lds((const void *)k_bark_uniform<false>, p.barkLds)); }
    if (p.aside) {
        CK(hipEventRecord(sy.noiseFork, st));
        CK(hipStreamWaitEvent(sy.side3, sy.noiseFork, 0));
        if (cplxChunked) CK(hipStreamWaitEvent(sy.side3, sy.cplxChunksDone, 0));
        else hipLaunchKernelGGL(k_cplx, dim3((p.NB + 63) / 64), dim3(64), 0, sy.side3, c, 0, c.K);
        CK(hipEventRecord(sy.cplxDone, sy.side3));
        MARK(mk, st);
        // the state for the next call only needs the transform to be done with the history: off the main stream
        launch_state_update(c, sy.side3);
        CK(hipEventRecord(sy.stateDone, sy.side3));
        CK(hipStreamWaitEvent(sy.side2, sy.noiseFork, 0));
        launch_noise(c, p, sy.side2);
        CK(hipEventRecord(sy.noiseDone, sy.side2));
    } else { hipLaunchKernelGGL(k_cplx, dim3((p.NB + 63) / 64), dim3(64), 0, st, c, 0, c.K);                MARK(mk, st); }
    const bool uniP = c.barkRing != 0;                      // masking sums of the un-decimated blocks on the geometry-uniform kernel too
    if (uniP) {
        hipLaunchKernelGGL(k_bark_uniform<false>, dim3((p.NB + 63) / 64), dim3(256), p.barkLds, st, c);
        hipLaunchKernelGGL(k_bark_levels<false>, dim3((unsigned)(((size_t)p.NB * 32 + WG - 1) / WG)), dim3(WG), 0, st, c);
    }
    hipLaunchKernelGGL(k_pbark, dim3((p.NB * 4 + 63) / 64), dim3(64), 0, st, c, uniP ? 1 : 0);            MARK(mk, st);
    // ("k_mask": gone - the masking level per line is formed where the keys are, mask_level(); geometries on the generic
    //  selection kernel evaluate it per key)
    MARK(mk, st);
    if (p.aside) CK(hipStreamWaitEvent(st, sy.cplxDone, 0));
    return ULCX_OK;
}

// One selection pass.  Per-stream rates: the probes select the searching blocks (pass 1, 2); the final pass selects them from
// their stored keys (pass 2) and then the VBR blocks as a one-pass call does (pass 0).
static int launch_select_wave(const UlcxEncCtx &c, const EncPlan &p, hipStream_t st, bool rates, int pass, int fin) {
    const PassKernel fn = select_fn(c, p.selPair, rates, pass);
    TRY(allow_lds((const void *)fn, p.selLds));
    if (p.selPair) hipLaunchKernelGGL(fn, dim3(p.NB), dim3(128), p.selLds, st, c, fin);           // one block per workgroup
    else hipLaunchKernelGGL(fn, dim3((p.NB + 3) / 4), dim3(256), p.selLds, st, c, fin);           // four
    return ULCX_OK;
}
static int launch_select(const UlcxEncCtx &c, const EncPlan &p, hipStream_t st, int fin) {
    if (!p.selWave) { hipLaunchKernelGGL(k_select, dim3(p.NB), dim3(WG), 0, st, c, fin); return ULCX_OK; }
    const bool rates = c.rates && c.selPass;
    TRY(launch_select_wave(c, p, st, rates, c.selPass, fin));
    if (rates && fin) TRY(launch_select_wave(c, p, st, true, 0, fin));
    return ULCX_OK;
}

// One encode pass over the blocks cc.fbMode picks, on s2: the main path (fbMode 1, the caller's stream) or the exact path's
// few blocks (fbMode 2: small grids that walk the list of owned blocks).
static int launch_encode(const UlcxEncCtx &cc, const EncPlan &p, UlcxEncSync &sy, hipStream_t s2, int fin, StageMarks &mk) {
    const bool fb2 = (cc.fbMode == 2);
    const int NB = p.NB, fbW = NB < 128 ? NB : 128;
    if (cc.useGapSums) {
        const size_t glds = nsums_lds_bytes(p.N, cc.C);
        TRY(allow_lds((const void *)k_nsums, glds));
        // the two speculative-sum kernels are independent: on the main path the tail chains run on a side stream beside the gaps
        const bool tailAside = !fb2 && p.aside;
        const unsigned tg = (unsigned)((p.nUnits + TAILS_U - 1) / TAILS_U);
        if (tailAside) {
            CK(hipEventRecord(sy.tailFork, s2));
            CK(hipStreamWaitEvent(sy.side2, sy.tailFork, 0));
            hipLaunchKernelGGL(k_tails, dim3(tg), dim3(WG), 0, sy.side2, cc, fin);
            CK(hipEventRecord(sy.tailDone, sy.side2));
        }
        const int nsGrid = NB < p.nsSlots ? NB : p.nsSlots;                 // persistent: what the device holds at once
        hipLaunchKernelGGL(k_nsums, dim3(fb2 ? fbW : nsGrid), dim3(WG), glds, s2, cc, fin);
        MARK(mk, s2);
        if (tailAside) CK(hipStreamWaitEvent(s2, sy.tailDone, 0));
        else hipLaunchKernelGGL(k_tails, dim3(fb2 ? fbW : tg), dim3(WG), 0, s2, cc, fin);
        MARK(mk, s2);
    } else { MARK(mk, s2); MARK(mk, s2); }
    if (cc.useWave) {
        const int nBC = NB * cc.C;
        hipLaunchKernelGGL(k_encode_wave<true>, dim3(fb2 ? fbW : (nBC + 3) / 4), dim3(256), (size_t)wavecaps_lds(p.capS) * 4 + 16, s2, cc, fin, p.capS, p.haveFull ? 0 : 2);
        if (p.haveFull) {
            // what the small capacities gave up on.  (The exact path's few blocks also retry with the medium capacities: a
            //  full-capacity workgroup needs a whole CU's LDS and would wait for the main path's kernel to drain)
            const WaveCaps capR = (p.haveMid && (fb2 || (p.probes > 0 && !fin))) ? p.capM : p.capF;
            hipLaunchKernelGGL(k_encode_wave<false>, dim3(fb2 ? fbW : ((nBC + 3) / 4 < 512 ? (nBC + 3) / 4 : 512)), dim3(256), (size_t)wavecaps_lds(capR) * 4 + 16, s2, cc, fin, capR, 1);
        }
    }
    MARK(mk, s2);
    hipLaunchKernelGGL(k_encode_units, dim3(fb2 ? fbW : (p.nUnits + 63) / 64), dim3(64), 0, s2, cc, fin);
    MARK(mk, s2);
    if (!fin && !fb2) hipLaunchKernelGGL(k_rate_step, dim3((NB + 255) / 256), dim3(256), 0, s2, cc);
    else hipLaunchKernelGGL(k_pack, dim3(fb2 ? (fbW + 3) / 4 : (NB + 3) / 4), dim3(256), 0, s2, cc, fin);
    MARK(mk, s2);
    return ULCX_OK;
}

// Exact path for tie-straddle blocks (~4e-4 of all): ONE heapsort per block and call gives the full
// ranking, from which the block finishes its own rate search / final pass by lookup.  lo: first of the group of rank slots.
static UlcxEncCtx exact_ctx(const UlcxEncCtx &c, int lo) { UlcxEncCtx cf = c; cf.fbMode = 2; cf.fbLo = lo; cf.fbHi = lo + c.rankSlots; return cf; }
static void exact_sort(const UlcxEncCtx &c, const EncPlan &p, hipStream_t s2, int lo) {
    const UlcxEncCtx cf = exact_ctx(c, lo);
    if (p.ldsEntries) hipLaunchKernelGGL(k_heapsel_pipe, dim3(p.fbGrid), dim3(64), p.heapLds, s2, cf, p.probes > 0 ? 1 : 0);
    else hipLaunchKernelGGL(k_heapsel, dim3(p.fbGrid), dim3(64), p.heapLds, s2, cf, p.ldsEntries);
}
static int exact_passes(const UlcxEncCtx &c, const EncPlan &p, UlcxEncSync &sy, hipStream_t s2, int lo) {
    const UlcxEncCtx cf = exact_ctx(c, lo);
    StageMarks none = { nullptr, 0 };
    for (int pass = 0; pass <= p.probes; pass++) {
        const int fin = (pass == p.probes) ? 1 : 0;
        // (one-pass calls: k_heapsel_pipe has written the kept set, and for the first group of rank slots k_cplx cleared the counter)
        const bool fromSort = (p.probes == 0 && p.ldsEntries);
        if (!fromSort) hipLaunchKernelGGL(k_keep_ranks, dim3(p.fbGrid), dim3(WG), 0, s2, cf, fin);
        if (cf.useWave && !(fromSort && lo == 0)) CK(hipMemsetAsync(cf.slow + p.NB + 1, 0, sizeof(int), s2));      // its own retry-queue counter
        TRY(launch_encode(cf, p, sy, s2, fin, none));
    }
    return ULCX_OK;
}

// The pass loop of one rate setting over the call's intermediates: the probes of a rate search (none for VBR) and the final
// pass, the exact path beside the final pass or behind the loop.  first: the call's first setting - its first pass carries
// the stage events and is where the noise log-spectrum joins (or, without side streams, runs).
static int launch_passes(UlcxEncCtx &c, const EncPlan &p, UlcxEncSync &sy, hipStream_t st, StageMarks &mk, bool first) {
    const int NB = p.NB;
    StageMarks none = { nullptr, 0 };
    // (c.fbCount, c.isFb and the first pass's c.slow are cleared by k_cplx; for a further rung of a ladder call by k_rung_arm)
    // The exact path forks at the FINAL pass (a block can first straddle there) and runs on a side stream beside the main
    // path's final encode: VBR has only that pass; CBR/ABR blocks replay their whole search from the ranking there.
    // Without side streams it runs behind the lock-step passes on the caller's stream.
    for (int pass = 0; pass <= p.probes; pass++) {
        const int fin = (pass == p.probes) ? 1 : 0;
        StageMarks &m = (pass == 0) ? mk : none;               // stage events: the first pass only
        const bool async_fb = p.aside && fin;
        if (c.useWave && pass > 0) CK(hipMemsetAsync(c.slow, 0, sizeof(int) * ((size_t)NB + 2), st));
        c.selPass = (p.probes > 0 && !c.keyFinal) ? (pass == 0 ? 1 : 2) : 0;
        TRY(launch_select(c, p, st, fin));
        MARK(m, st);
        if (async_fb) {
            CK(hipEventRecord(sy.exactFork, st));
            CK(hipStreamWaitEvent(sy.side, sy.exactFork, 0));
            exact_sort(c, p, sy.side, 0);                      // needs only the keys: starts right behind the select
        }
        if (pass == 0) {
            if (first) {
                if (p.aside) CK(hipStreamWaitEvent(st, sy.noiseDone, 0));   // (k_nbark / k_nline intervals: hidden)
                else launch_noise(c, p, st);
            }
            MARK(m, st); MARK(m, st);
        }
        if (async_fb) {
            CK(hipEventRecord(sy.exactFork2, st));              // the exact path's encode pass needs the noise pairs too
            CK(hipStreamWaitEvent(sy.side, sy.exactFork2, 0));
            TRY(exact_passes(c, p, sy, sy.side, 0));
            for (int lo = c.rankSlots; lo < NB; lo += c.rankSlots) {
                exact_sort(c, p, sy.side, lo);
                TRY(exact_passes(c, p, sy, sy.side, lo));
            }
            CK(hipEventRecord(sy.exactJoin, sy.side));
        }
        MARK(m, st);                                           // ("k_heapsel": empty interval on the main stream)
        UlcxEncCtx cm = c; cm.fbMode = 1;
        TRY(launch_encode(cm, p, sy, st, fin, m));
        if (async_fb) CK(hipStreamWaitEvent(st, sy.exactJoin, 0));
    }
    if (!p.aside) {
        for (int lo = 0; lo < NB; lo += c.rankSlots) {
            exact_sort(c, p, st, lo);
            TRY(exact_passes(c, p, sy, st, lo));
        }
    }
    return ULCX_OK;
}

// One call under nRungs rate settings (ulcx_encode_*_ladder; a plain call is one rung).  The contexts differ in the setting
// (mode / p0 / p1 / vbrTarget / rates) and in where the blocks and sizes go (out / bits).  Rung 0 is the call as it always
// was: front half, sums and levels, then its passes - armed by k_cplx.  Every further rung is armed by k_rung_arm and runs
// the pass loop again over the same intermediates, behind the previous rung's last kernel on the caller's stream and behind
// its exact path's join: the arming clears what that path still reads.  The noise log-spectrum joins once (rung 0), the
// state for the next call behind the last rung.
int ulcx_enc_launch_ladder(const UlcxEncCtx *rungs, int nRungs, hipStream_t st, hipEvent_t *ev, const UlcxEncAux &aux) {
    UlcxEncCtx c = rungs[0];                                   // (keyFinal, selPass are set below)
    UlcxEncSync &sy = aux.sync;
    const EncPlan p = enc_plan(c, aux);
    StageMarks mk = { ev, 0 }, none = { nullptr, 0 };
    if (p.probes) CK(hipMemsetAsync(c.cbrLive, 0, sizeof(int), st));
    if (c.barkRing) CK(hipMemsetAsync(c.decCount, 0, sizeof(int), st));           // k_xf lists this call's decimated blocks
    if (nRungs > 1) CK(hipMemsetAsync(c.fbCount + 1, 0, sizeof(int), st));        // exact-path blocks of the rungs in front of the last
    MARK(mk, st);
    // --- window control + transform
    TRY(launch_front(c, st, mk, aux, ULCX_FRONT_ENCODE));
    if (ULCX_DBG(c) & 0x6000) { MARK(mk, st); return ULCX_OK; }     // (ablation build: stop behind window control / transform)
    // --- sums, masking levels; the noise log-spectrum beside them (it does not feed the keys)
    TRY(launch_psy(c, p, sy, st, mk, aux.wcPipe > 1));
    // --- selection + encode pass(es)
    // geometries the one-wave-per-block selection does not cover go through the multi-pass kernel, which reads every
    // key several times: form the final keys once for it (and for the exact path's heapsort) - once per call, not per rung
    if (!p.selWave) { ulcx_enc_finalize_keys(c, st); c.keyFinal = 1; }
    TRY(allow_lds((const void *)k_heapsel, p.heapLds)); TRY(allow_lds((const void *)k_heapsel_pipe, p.heapLds));
    if (p.haveFull && (size_t)wavecaps_lds(p.capF) * 4 > 48 * 1024) CK(hipFuncSetAttribute((const void *)k_encode_wave<false>, hipFuncAttributeMaxDynamicSharedMemorySize, wavecaps_lds(p.capF) * 4 + 16));
    TRY(launch_passes(c, p, sy, st, mk, true));
    for (int r = 1; r < nRungs; r++) {
        UlcxEncCtx cr = rungs[r];
        cr.keyFinal = c.keyFinal;
        EncPlan pr = p;
        pr.probes = enc_probes(cr, p.N);
        if (pr.probes) CK(hipMemsetAsync(cr.cbrLive, 0, sizeof(int), st));
        ulcx_enc_rung_arm(cr, st);
        TRY(launch_passes(cr, pr, sy, st, none, false));
    }
    MARK(mk, st);   // cbr_probe_passes (empty interval for VBR; a ladder call: every pass behind rung 0's first)
    if (p.aside) CK(hipStreamWaitEvent(st, sy.stateDone, 0));
    else launch_state_update(c, st);
    MARK(mk, st);
    CK(hipGetLastError());
    return ULCX_OK;
}

int ulcx_enc_launch(const UlcxEncCtx &c, hipStream_t st, hipEvent_t *ev, const UlcxEncAux &aux) {
    return ulcx_enc_launch_ladder(&c, 1, st, ev, aux);
}

// The analysis call (ulcx_analyse_dev): the front half of an encode call - window control in the same steps over the same side
// streams, then per transform chunk the MDCT-only transform and the chunk's ordered sums beside the next chunk - and the
// state for the next call.  No Bark sums, selection, noise sums, tails or writer, no counter of the encode call is touched.
// Every side stream is joined back into st: side through the sums' event, side2 and side3 through the last decide step the
// last transform chunk waits for.
int ulcx_analyse_launch(const UlcxEncCtx &c, hipStream_t st, hipEvent_t *ev, const UlcxEncAux &aux, int useKxf) {
    const int what = !c.cplxOut ? ULCX_FRONT_WC_ONLY : useKxf ? ULCX_FRONT_ANALYSE_KXF : ULCX_FRONT_ANALYSE;
    if (what == ULCX_FRONT_ANALYSE_KXF && c.barkRing) CK(hipMemsetAsync(c.decCount, 0, sizeof(int), st));   // (k_xf lists the decimated blocks)
    StageMarks mk = { ev, 0 };
    MARK(mk, st);
    TRY(launch_front(c, st, mk, aux, what));
    if (aux.wcPipe > 1) CK(hipStreamWaitEvent(st, aux.sync.cplxChunksDone, 0));          // the chunks' sums (on the first side stream)
    else hipLaunchKernelGGL(k_cplxa, dim3((c.B * c.K + 63) / 64), dim3(64), 0, st, c, 0, c.K);
    MARK(mk, st);                                              // k_cplx
    while (mk.ev && mk.stage < ULCX_ENC_STAGES) MARK(mk, st);  // (the back half: empty intervals)
    launch_state_update(c, st);
    MARK(mk, st);
    CK(hipGetLastError());
    return ULCX_OK;
}
