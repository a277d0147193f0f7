// ulcx_tables.cpp — host construction of the data-independent tables the kernels read
// (SURVEY.md Appendix C.6).  Everything here is evaluated ONCE per encoder/decoder with
// the HOST libm, exactly where the reference evaluates it per block with the same
// arguments:
//   Bark band edges / per-line Bark position : libulc/ulcEncoder_Psyopt.c:109-116,141-143,198-205,237-239
//                                              via libulc/ulcHelper.h:96-120
//   DCT-IV / FFT twiddles, sine-window ramps : "fourier spec v2" (FormatSpecs.md:155)
// so that the device never needs sinhf/asinhf/cos/sin.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ulcx_internal.h"

static thread_local char g_err[512] = "";
void ulcx_set_error(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *ulcx_last_error(void) { return g_err; }

// ulcHelper.h:96-120 (binary32 expressions, same operation order)
static float freq_to_line(float hz, float nyq, uint32_t n) { return (hz * (float)n / nyq) - 0.5f; }
static float line_to_freq(uint32_t line, float nyq, uint32_t n) { return ((float)line + 0.5f) * nyq / (float)n; }
static float freq_to_bark(float hz) { return 6.0f * asinhf(hz * (1.0f / 600.0f)); }
static float bark_to_freq(float bark) { return 600.0f * sinhf(bark * (1.0f / 6.0f)); }

static void band_edges(short *beg, short *end, int nLines, float nyq, float offLo, float offHi) {
    for (int b = 0; b < ULCX_NBARK; b++) {
        float f0 = bark_to_freq((float)b + offLo);
        float f1 = bark_to_freq((float)b + offHi);
        int l0 = (int)floorf(freq_to_line(f0, nyq, (uint32_t)nLines));
        int l1 = (int)ceilf(freq_to_line(f1, nyq, (uint32_t)nLines));
        if (l0 < 0) l0 = 0;
        if (l1 < 0) l1 = 0;
        if (l0 > nLines - 1) l0 = nLines - 1;
        if (l1 > nLines) l1 = nLines;
        beg[b] = (short)l0; end[b] = (short)l1;
    }
}

// The band tables of every subblock size, into T: the one place they are formed (the encoder's create call through
// tables_host, ulcx_debug_band_plan directly)
static void band_tables(UlcxTables *T, int BS, int rateHz) {
    const float nyq = (float)rateHz * 0.5f;
    for (int d = 0; d < ULCX_MAX_SUB; d++) {
        const int nLines = (BS >> d) / 2;
        band_edges(T->nBeg[d], T->nEnd[d], nLines, nyq, 0.0f, 2.0f);
        band_edges(T->pBeg[d], T->pEnd[d], nLines, nyq, -0.75f, 0.25f);
    }
}

// k_bark_uniform: the band edges of a subblock size as one list in line order, [noise|psycho][d][ULCX_BARK_EVENTS] words
// line | kind << 16 | band << 24 (kind 0: lower edge, 1: upper edge, 2: end of the subblock); at equal lines lower
// edges come first (a band of no lines opens, then closes)
static void band_events(const UlcxTables *T, int BS, uint32_t *sch) {
    for (int t = 0; t < 2; t++) for (int d = 0; d < ULCX_MAX_SUB; d++) {
        const short *beg = t ? T->pBeg[d] : T->nBeg[d], *end = t ? T->pEnd[d] : T->nEnd[d];
        uint32_t *o = sch + (size_t)(t * ULCX_MAX_SUB + d) * ULCX_BARK_EVENTS;
        int n = 0, bo = 0, bc = 0, N = (BS >> d) / 2;
        bool ordered = true;
        for (int b = 0; b < ULCX_NBARK; b++) {
            if (beg[b] > end[b] || end[b] > N) ordered = false;
            if (b && (beg[b] < beg[b - 1] || end[b] < end[b - 1])) ordered = false;
        }
        if (ordered) while (bc < ULCX_NBARK) {
            int pos = (bo < ULCX_NBARK && beg[bo] <= end[bc]) ? beg[bo] : end[bc];
            while (bo < ULCX_NBARK && beg[bo] == pos) { o[n++] = (uint32_t)pos | (0u << 16) | ((uint32_t)bo << 24); bo++; }
            while (bc < bo && end[bc] == pos) { o[n++] = (uint32_t)pos | (1u << 16) | ((uint32_t)bc << 24); bc++; }
        }
        o[n++] = (uint32_t)N | (2u << 16);
        while (n < ULCX_BARK_EVENTS) o[n++] = 0xffffu | (3u << 16);
    }
}

// k_bark_uniform keeps one snapshot of the running sums per Bark band that is open (lower edge passed, upper edge not yet):
// the most the full-size band tables ever have open at once sizes its ring.  0: k_nbark / k_pbark for every block - geometries
// whose band edges need a deeper ring than 8.
int ulcx_tables_bark_ring(const UlcxTables &T, int BS, int *mostOpen) {
    int most = 0;
    const int N = BS / 2;
    for (int t = 0; t < 2; t++) {
        const short *beg = t ? T.pBeg[0] : T.nBeg[0], *end = t ? T.pEnd[0] : T.nEnd[0];
        for (int b = 0; b < ULCX_NBARK; b++) {
            if (beg[b] > end[b] || end[b] > N) most = 1 << 20;
            if (b && (beg[b] < beg[b - 1] || end[b] < end[b - 1])) most = 1 << 20;
        }
        for (int pos = 0; pos <= N; pos++) {
            int open = 0;
            for (int b = 0; b < ULCX_NBARK; b++) open += (beg[b] <= pos && pos <= end[b]) ? 1 : 0;
            if (open > most) most = open;
        }
    }
    int ring = 4;
    while (ring < most) ring *= 2;
    if (mostOpen) *mostOpen = most;
    return (ring <= 8 && N % 32 == 0) ? ring : 0;
}

// Test hooks, host arithmetic only (include/ulc_amd.h)
static int band_args_bad(const char *who, int BS, int rateHz, const void *out) {
    if (out && BS >= 256 && BS <= ULCX_MAX_BS_DEVICE && (BS & (BS - 1)) == 0 && rateHz >= 1) return 0;
    ulcx_set_error("%s: no array, or BlockSize %d / RateHz %d not an encoder's", who, BS, rateHz);
    return 1;
}
extern "C" int ulcx_debug_band_plan(int BlockSize, int RateHz, int16_t *edges, int32_t *most, int32_t *ring) {
    if (band_args_bad("ulcx_debug_band_plan", BlockSize, RateHz, edges)) return ULCX_ERR_ARG;
    UlcxTables T;
    memset(&T, 0, sizeof(T));
    band_tables(&T, BlockSize, RateHz);
    const size_t n = (size_t)ULCX_MAX_SUB * ULCX_NBARK;
    for (int d = 0; d < ULCX_MAX_SUB; d++) for (int b = 0; b < ULCX_NBARK; b++) {
        int16_t *o = edges + (size_t)d * 2 * ULCX_NBARK + b;
        o[0] = T.nBeg[d][b]; o[ULCX_NBARK] = T.nEnd[d][b];
        o[2 * n] = T.pBeg[d][b]; o[2 * n + ULCX_NBARK] = T.pEnd[d][b];
    }
    int m = 0;
    const int r = ulcx_tables_bark_ring(T, BlockSize, &m);
    if (most) *most = m;
    if (ring) *ring = r;
    return ULCX_OK;
}
extern "C" int ulcx_debug_band_events(int BlockSize, int RateHz, uint32_t *events) {
    if (band_args_bad("ulcx_debug_band_events", BlockSize, RateHz, events)) return ULCX_ERR_ARG;
    UlcxTables T;
    memset(&T, 0, sizeof(T));
    band_tables(&T, BlockSize, RateHz);
    band_events(&T, BlockSize, events);
    return ULCX_OK;
}

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

// The tables as the device will hold them: one host blob and the offsets of its parts (tables_host), then the copy (ulcx_tables_build)
namespace { struct TablesHost {
    std::vector<unsigned char> blob;
    size_t offPre[ULCX_MAX_SUB], offTw[ULCX_MAX_SUB], offIdx[ULCX_MAX_SUB], offFrac[ULCX_MAX_SUB], offW[ULCX_MAX_SUB], offFall, offRise, offSched;
}; }
static void tables_host(UlcxTables *T, TablesHost &H, int BS, int rateHz, bool forEncoder) {
    memset(T, 0, sizeof(*T));
    std::vector<unsigned char> &blob = H.blob;
    auto reserve = [&](size_t bytes) { size_t off = (blob.size() + 255) & ~(size_t)255; blob.resize(off + bytes); return off; };
    size_t *offPre = H.offPre, *offTw = H.offTw, *offIdx = H.offIdx, *offFrac = H.offFrac, *offW = H.offW;
    for (int d = 0; d < ULCX_MAX_SUB; d++) offW[d] = 0;
    float nyq = (float)rateHz * 0.5f;
    for (int d = 0; d < ULCX_MAX_SUB; d++) {
        int S = BS >> d, M = S / 2;
        offPre[d] = reserve(sizeof(float2) * M);
        offTw[d]  = reserve(sizeof(float2) * (M / 2 + 1));
        float2 *pre = (float2 *)(blob.data() + offPre[d]);
        for (int n = 0; n < M; n++) {
            double th = M_PI * (double)(8 * n + 1) / (double)(8 * S);
            pre[n].x = (float)cos(th); pre[n].y = (float)sin(th);
        }
        float2 *tw = (float2 *)(blob.data() + offTw[d]);
        for (int j = 0; j < M / 2; j++) {
            double th = 2.0 * M_PI * (double)j / (double)M;
            tw[j].x = (float)cos(th); tw[j].y = (float)sin(th);
        }
        if (forEncoder) {
            int nLines = S / 2;
            offIdx[d]  = reserve(sizeof(int) * nLines);
            offFrac[d] = reserve(sizeof(float) * nLines);
            int *bi = (int *)(blob.data() + offIdx[d]);
            float *fr = (float *)(blob.data() + offFrac[d]);
            for (int line = 0; line < nLines; line++) {
                float bb = freq_to_bark(line_to_freq((uint32_t)line, nyq, (uint32_t)nLines));
                int i = (int)bb;
                bi[line] = i;
                fr[line] = bb - (float)i;
            }
            {
                offW[d] = reserve(sizeof(float) * 4 * nLines);
                float *w0 = (float *)(blob.data() + offW[d]);
                bi = (int *)(blob.data() + offIdx[d]); fr = (float *)(blob.data() + offFrac[d]);      // (reserve() may have moved the blob)
                for (int line = 0; line < nLines; line++) {
                    const int iL = bi[line] < ULCX_NBARK ? bi[line] : ULCX_NBARK - 1;                   // Psyopt.c:143-147
                    const int iR = bi[line] + 1 < ULCX_NBARK ? bi[line] + 1 : iL;
                    memcpy(&w0[4 * line + 0], &iL, 4); memcpy(&w0[4 * line + 1], &iR, 4);
                    w0[4 * line + 2] = 1.0f - fr[line]; w0[4 * line + 3] = fr[line];
                }
            }
        }
    }
    if (forEncoder) band_tables(T, BS, rateHz);
    // window ramps: overlap Ov = 2^j stored at [Ov, 2 Ov)
    size_t offFall = reserve(sizeof(float) * 2 * BS), offRise = reserve(sizeof(float) * 2 * BS);
    {
        float *fall = (float *)(blob.data() + offFall), *rise = (float *)(blob.data() + offRise);
        for (int ov = 1; ov <= BS; ov <<= 1)
            for (int i = 0; i < ov; i++) {
                double th = M_PI * (double)(2 * i + 1) / (double)(4 * ov);
                fall[ov + i] = (float)cos(th);
                rise[ov + i] = (float)sin(th);
            }
    }
    const size_t offSched = reserve(sizeof(uint32_t) * 2 * ULCX_MAX_SUB * ULCX_BARK_EVENTS);
    if (forEncoder) band_events(T, BS, (uint32_t *)(blob.data() + offSched));
    H.offFall = offFall; H.offRise = offRise; H.offSched = offSched;
}

int ulcx_tables_build(UlcxTables *T, void **devBlob, int BS, int rateHz, bool forEncoder) {
    TablesHost H;
    tables_host(T, H, BS, rateHz, forEncoder);
    const std::vector<unsigned char> &blob = H.blob;
    const size_t *offPre = H.offPre, *offTw = H.offTw, *offIdx = H.offIdx, *offFrac = H.offFrac, *offW = H.offW;
    const size_t offFall = H.offFall, offRise = H.offRise, offSched = H.offSched;
    void *dev = nullptr;
    hipError_t e = hipMalloc(&dev, blob.size());
    if (e != hipSuccess) { ulcx_set_error("hipMalloc(tables): %s", hipGetErrorString(e)); return ULCX_ERR_NOMEM; }
    e = hipMemcpy(dev, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { ulcx_set_error("hipMemcpy(tables): %s", hipGetErrorString(e)); hipFree(dev); return ULCX_ERR_HIP; }
    unsigned char *base = (unsigned char *)dev;
    for (int d = 0; d < ULCX_MAX_SUB; d++) {
        T->pre[d] = (const float2 *)(base + offPre[d]);
        T->tw[d]  = (const float2 *)(base + offTw[d]);
        if (forEncoder) {
            T->bandIdx[d]  = (const int *)(base + offIdx[d]);
            T->bandFrac[d] = (const float *)(base + offFrac[d]);
            T->bandW[d]    = (const float4 *)(base + offW[d]);
        }
    }
    T->barkSched = (const uint32_t *)(base + offSched);
    T->winFall = (const float *)(base + offFall);
    T->winRise = (const float *)(base + offRise);
    *devBlob = dev;
    return ULCX_OK;
}
