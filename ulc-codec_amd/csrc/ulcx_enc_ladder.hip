// ulcx_enc_ladder.hip - the ladder call's own device code (ulcx_encode_*_ladder): arming a further rung.
//
// A ladder call encodes the same blocks under several rate settings.  Everything in front of the selection - window control,
// transform, ordered sums, Bark levels, the noise log-spectrum, the state for the next call - runs once, for rung 0, whose
// k_cplx also arms rung 0's rate logic.  Every further rung re-runs the back half (selection + writer passes) over the same
// intermediates; k_rung_arm puts the per-block rate state where k_cplx leaves it for a call's first pass.
// A translation unit of its own: nothing here is instantiated beside k_xf / k_cplx, whose schedules must not move.
#include "ulcx_enc_dev.h"

// What k_cplx does from the rate lookup on (ulcx_enc_xf.hip), for the setting in this rung's context, from the three values the
// front half leaves behind: BlockComplexity (c.cplx), the non-zero coefficient count (c.nnz) and - recounted here, only by
// blocks that search - the number of collapsible coefficients.  One lane per block.
__global__ __launch_bounds__(64) void k_rung_arm(UlcxEncCtx c) {
    const int blk = blockIdx.x * 64 + threadIdx.x;
    if (blk >= c.B * c.K) return;
    int mode = c.mode;
    float p0 = c.p0, p1 = c.p1, vbrTarget = c.vbrTarget;
    if (c.rates) {
        const float2 r = c.rates[blk / c.K];
        if (r.x < 0.0f) {
            mode = ULCX_MODE_VBR; p0 = -r.x;
            vbrTarget = 0x1.E4EFB7p3f * ulcx_logf(100.0f / p0);       // ulcEncoder.c:144 (correctly rounded division, glibc logf)
        } else { mode = (r.y > 0.0f) ? ULCX_MODE_ABR : ULCX_MODE_CBR; p0 = r.x; p1 = r.y; }
    }
    const float cx = c.cplx[blk];
    const int maxCoef = c.nnz[blk];
    if (mode == ULCX_MODE_VBR) {
        int nT = maxCoef;
        if (vbrTarget > 0.0f) {
            float ft = (c.C * c.BS) * cx / vbrTarget;
            if (ft < maxCoef) nT = (int)ft;
        }
        c.nout[blk] = nT;
        if (c.rates) {
            // (a VBR block beside searching ones: the state k_cplx gives it)
            c.cbrLo[blk] = 0; c.cbrHi[blk] = maxCoef;
            c.cbrDone[blk] = ULCX_DONE_VBR;
            c.cbrBudget[blk] = 0;
            c.selWin[blk] = make_uint4(0u, 0u, (uint32_t)(c.C * c.BS), 0u);
            for (int u = 0; u < c.C * 4; u++) c.tailSum[((size_t)blk * c.C * 4 + u) * 8 + 6] = 0.0f;
        }
    } else {
        // non-zero coefficients the coarsest quantizer could collapse (Encode.c:114): an integer count, any order
        int tiny = 0;
        const int n = c.C * c.BS;
        const float4 *p = (const float4 *)(c.coef + (size_t)blk * n);
        for (int i = 0; i < n / 4; i += 4) {
            float4 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) q[u] = p[i + u];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const float4 v = q[u];
                tiny += (fabsf(v.x) >= 0.5f * ULCX_COEF_EPS && fabsf(v.x) < 0x1.0p-29f) ? 1 : 0;
                tiny += (fabsf(v.y) >= 0.5f * ULCX_COEF_EPS && fabsf(v.y) < 0x1.0p-29f) ? 1 : 0;
                tiny += (fabsf(v.z) >= 0.5f * ULCX_COEF_EPS && fabsf(v.z) < 0x1.0p-29f) ? 1 : 0;
                tiny += (fabsf(v.w) >= 0.5f * ULCX_COEF_EPS && fabsf(v.w) < 0x1.0p-29f) ? 1 : 0;
            }
        }
        // CBR/ABR binary search state (ulcEncoder.c:96-101), probes that are over budget for certain taken at once (k_cplx)
        float kbps = p0;
        if (mode == ULCX_MODE_ABR) kbps = p0 * cx / p1;
        const int budget = (int)((c.BS * kbps) * 1000.0f / c.rateHz);
        int lo = 0, hi = maxCoef;
        int done = (0 < maxCoef) ? 0 : 1;
        int nOut = (0 < maxCoef) ? (int)((unsigned)(0 + maxCoef) / 2u) : 0;
        while (!done && 4 * (nOut - tiny + 1) > budget) {
            hi = nOut - 1;
            if (!(lo < hi - 1)) { done = 1; nOut = lo; }
            else nOut = (int)((unsigned)(lo + hi) / 2u);
        }
        c.cbrLo[blk] = lo; c.cbrHi[blk] = hi;
        c.cbrDone[blk] = done;
        c.selWin[blk] = make_uint4(0u, 0u, (uint32_t)(c.C * c.BS), 0u);
        for (int u = 0; u < c.C * 4; u++) c.tailSum[((size_t)blk * c.C * 4 + u) * 8 + 6] = 0.0f;
        {   // rate searches still open: one add per wave (the launcher has cleared the word)
            const unsigned long long open = __ballot(!done);
            if (open && (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(open >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)open, 0u)) == 0 && !done)
                atomicAdd(c.cbrLive, (int)__popcll(open));
        }
        c.nout[blk] = nOut;
        c.cbrBudget[blk] = budget;
    }
    // the per-call flags as a call's first pass finds them; the exact-path count of the rungs so far moves to the second word
    // of c.fbCount (ulcx_encoder_last_fallbacks reports the sum)
    c.isFb[blk] = 0;
    if (c.useWave) c.slow[blk] = 0;
    if (blk == 0) {
        c.fbCount[1] += c.fbCount[0]; c.fbCount[0] = 0;
        if (c.useWave) { c.slow[c.B * c.K] = 0; c.slow[c.B * c.K + 1] = 0; }
    }
}

void ulcx_enc_rung_arm(const UlcxEncCtx &c, hipStream_t st) {
    hipLaunchKernelGGL(k_rung_arm, dim3((unsigned)((c.B * c.K + 63) / 64)), dim3(64), 0, st, c);
}
