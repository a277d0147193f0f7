/*
 * ulcx_tool.c — batched front-end over libulc_amd.so.
 *
 *   ulcx-tool encode OUTDIR RATE[,AvgComplexity] [-blocksize:N] [-devices:N] [-index] IN1.wav [-rate:RATE[,AvgComplexity]] IN2.wav ...
 *   ulcx-tool decode OUTDIR [-format:PCM16|FLOAT32] [-blocks:FIRST,COUNT] [-devices:N] IN1.ulc IN2.ulc ...
 *   ulcx-tool analyse [-blocksize:N] [-devices:N]                            IN1.wav IN2.wav ...
 *
 * What tools/ulcEncodeTool.c / tools/ulcDecodeTool.c of the reference do for ONE file per
 * process, done for MANY files per call: every input is one stream of the batch, all streams
 * advance K blocks per library call.  RATE follows the reference's convention
 * (ulcEncodeTool.c:38-50): negative = VBR quality, positive = CBR kbps, "kbps,complexity" = ABR.
 * Files may have settings of their own in one batch: "-rate:RATE[,AvgComplexity]" among the inputs sets the
 * rate of the inputs that follow it (the positional RATE is the default; per-stream table of
 * ulcx_encode_host_rates), e.g. `ulcx-tool encode out -50 a.wav -rate:48 b.wav -rate:96,0.41 c.wav`.
 * "RATE,auto" (positional or -rate:) is the reference's two-run ABR workflow in one command: an
 * analysis pass (ulcx_analyse_host: no selection, no writer) sums each file's BlockComplexity
 * (ulcEncodeTool.c:164,178), then each file is encoded in ABR at its own average complexity, in CBR where
 * that is 0; its line reports the value used.  "analyse" runs that pass alone and prints per file the block
 * count, the average complexity `RATE,<complexity>` is to be fed with and the number of window-switched
 * blocks; it writes no file.
 * A ladder "R0/R1/.../Rn" (up to 8 rungs, each in RATE's syntax, `auto` included; positional and in every -rate:, all with
 * the same number of rungs) encodes every file under each rung in ONE library call per batch of blocks
 * (ulcx_encode_host_ladder: window control, transform and complexity once) and writes OUTDIR/stem.r<i>.ulc, i from 0, each
 * the file the reference's tool writes at Ri; `auto` rungs share one analysis pass.
 * Files written are byte-identical to the reference tools' (tests/test_gpu_dropin.py):
 * container layout tools/ulc_Helper.h:10-20, block count ulcEncodeTool.c:93-98 (+2 blocks of
 * coding/MDCT delay), sample conversion WavIO_Helper.c:49-63 (x 2^-15 in, lrintf(clamp(x 2^15)) out).
 * All inputs of one call must share rate / channel count (encode) or rate / channels / block size
 * (decode); inputs may have different lengths (shorter ones are padded with silence and trimmed
 * to their own block count on output).
 *
 * -blocks:FIRST,COUNT (decode): each output holds blocks FIRST .. FIRST+COUNT-1 of its file only (trimmed where the file's
 * header counts fewer), exactly the bytes a full decode writes for them: the payloads are indexed once on the device
 * (ulcx_decoder_index_resident), then decoded by range calls (ulcx_decode_resident_range_host) - nothing in front of FIRST
 * but one block is synthesised.
 *
 * -index (encode): a block index beside every file written - OUTDIR/stem.ulx, OUTDIR/stem.r<i>.ulx per rung of a ladder
 * (include/ulc_amd.h section 3, `.ulx`).  It grows with the encoder's output: after every encode call the call's blocks, still
 * in their slots, are indexed side by side (ulcx_index_slots_host, all rungs' rows in one call); the file is never walked.
 * decode -blocks: loads IN.ulx from beside IN.ulc when every input has one whose header agrees with the `.ulc` header and
 * which passes ulcx_index_check against the payload's size (ulcx_decoder_set_resident_index); otherwise it indexes the
 * payloads as before and says so on stderr.  The bytes written are the same either way.
 *
 * -devices:N (independent streams shard by plain batch split, one host thread per device, no collective): the
 * inputs are dealt round-robin over N groups, every group gets its own encoder / decoder and its own host thread; group g
 * runs on device g % (visible devices), so N may exceed the device count (two groups then share a GPU).  The files written
 * do not depend on N.
 *
 * WAV support is deliberately minimal: RIFF/WAVE, "fmt " PCM 16-bit or IEEE float 32-bit, one
 * "data" chunk.  Host code is plain C over the C ABI of include/ulc_amd.h.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/ulc_amd.h"

#define KBLOCKS 16                      /* blocks per stream per library call */

struct wav { int rate, chan, bits, isFloat; uint32_t nFrames; long dataOffs; FILE *f; };

static uint32_t rd32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }
static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | p[1] << 8); }

static int wav_open(struct wav *w, const char *path) {
    uint8_t h[12], ck[8], fmt[40];
    memset(w, 0, sizeof(*w));
    w->f = fopen(path, "rb");
    if (!w->f) return -1;
    if (fread(h, 1, 12, w->f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return -2;
    int haveFmt = 0;
    for (;;) {
        if (fread(ck, 1, 8, w->f) != 8) return -3;
        uint32_t sz = rd32(ck + 4);
        if (!memcmp(ck, "fmt ", 4)) {
            uint32_t n = sz < sizeof(fmt) ? sz : (uint32_t)sizeof(fmt);
            if (sz < 16 || fread(fmt, 1, n, w->f) != n) return -4;
            if (sz > n) fseek(w->f, (long)(sz - n), SEEK_CUR);
            int tag = rd16(fmt);
            if (tag == 0xFFFE && sz >= 26) tag = rd16(fmt + 24);          /* WAVE_FORMAT_EXTENSIBLE: sub-format */
            w->chan = rd16(fmt + 2); w->rate = (int)rd32(fmt + 4); w->bits = rd16(fmt + 14);
            w->isFloat = (tag == 3);
            if (!((tag == 1 && w->bits == 16) || (tag == 3 && w->bits == 32))) return -5;
            haveFmt = 1;
        } else if (!memcmp(ck, "data", 4)) {
            if (!haveFmt) return -6;
            w->dataOffs = ftell(w->f);
            w->nFrames = sz / (uint32_t)(w->chan * w->bits / 8);
            return 0;
        } else fseek(w->f, (long)(sz + (sz & 1)), SEEK_CUR);
    }
}
/* frames [pos, pos+n) as float, zero padded past the end (WavIO_Reader.c:115-150) */
static void wav_read(struct wav *w, uint32_t pos, uint32_t n, float *dst, void *tmp) {
    uint32_t have = pos < w->nFrames ? w->nFrames - pos : 0;
    if (have > n) have = n;
    size_t fb = (size_t)w->chan * w->bits / 8;
    if (have) {
        fseek(w->f, w->dataOffs + (long)(pos * fb), SEEK_SET);
        size_t got = fread(tmp, fb, have, w->f);
        if (got < have) have = (uint32_t)got;
    }
    size_t ns = (size_t)have * w->chan;
    if (w->isFloat) memcpy(dst, tmp, ns * 4);
    else { const int16_t *s = (const int16_t *)tmp; for (size_t i = 0; i < ns; i++) dst[i] = (float)s[i] * 0x1.0p-15f; }
    for (size_t i = ns; i < (size_t)n * w->chan; i++) dst[i] = 0.0f;
}
static void wav_write_header(FILE *f, int rate, int chan, int isFloat, uint32_t nFrames) {
    int bits = isFloat ? 32 : 16;
    uint32_t dataBytes = nFrames * (uint32_t)(chan * bits / 8);
    uint8_t h[44] = { 'R','I','F','F', 0,0,0,0, 'W','A','V','E', 'f','m','t',' ', 16,0,0,0 };
    uint32_t riff = 36 + dataBytes, bps = (uint32_t)(rate * chan * bits / 8);
    memcpy(h + 4, &riff, 4);
    h[20] = isFloat ? 3 : 1; h[22] = (uint8_t)chan; h[23] = (uint8_t)(chan >> 8);
    memcpy(h + 24, &rate, 4); memcpy(h + 28, &bps, 4);
    h[32] = (uint8_t)(chan * bits / 8); h[34] = (uint8_t)bits;
    memcpy(h + 36, "data", 4); memcpy(h + 40, &dataBytes, 4);
    fwrite(h, 1, 44, f);
}
static const char *base_name(const char *p) { const char *s = strrchr(p, '/'); return s ? s + 1 : p; }
static void out_path(char *dst, size_t n, const char *dir, const char *in, const char *ext) {
    char stem[512];
    snprintf(stem, sizeof(stem), "%s", base_name(in));
    char *dot = strrchr(stem, '.'); if (dot) *dot = 0;
    snprintf(dst, n, "%s/%s%s", dir, stem, ext);
}
#define DIE(...) do { fprintf(stderr, "ulcx-tool: " __VA_ARGS__); fprintf(stderr, "\n"); return 2; } while (0)

/* one group of inputs = one batch on one device (the whole command line, or a -devices:N share of it on its own thread);
 * encode: rung r of file i is encoded under {RateKbps, AvgComplexity} = setting[i * ULCX_MAX_RUNGS + r], r < nRungs;
 * autoc[...] = 1: "RATE,auto" (two passes) */
struct group { int decode, analyse, device, n; char **files; const char *outdir; ulcx_rate *setting; int *autoc; int nRungs; int bs, isFloat; int rc;
               int32_t rFirst, rCount; /* decode -blocks:FIRST,COUNT (rCount 0: whole files) */
               int index; /* encode -index: write stem.ulx beside every stem.ulc */ };

/* "RATE[,AvgComplexity]" or "RATE,auto", validated as ulcEncodeTool.c:43-50 does (and finite: the library refuses the rest) */
static int parse_rate(const char *s, ulcx_rate *r, int *isAuto) {
    r->RateKbps = 0.0f; r->AvgComplexity = 0.0f; *isAuto = 0;
    const char *comma = strchr(s, ',');
    if (comma && !strcmp(comma + 1, "auto")) { *isAuto = 1; if (sscanf(s, "%f", &r->RateKbps) != 1) return -1; }
    else if (sscanf(s, "%f,%f", &r->RateKbps, &r->AvgComplexity) < 1) return -1;
    if (!isfinite(r->RateKbps) || !isfinite(r->AvgComplexity) || r->RateKbps == 0.0f || r->AvgComplexity < 0.0f) return -1;
    if (*isAuto && r->RateKbps < 0.0f) return -1;                  /* ABR needs a rate in kbps */
    return 0;
}

/* A ladder "R0/R1/.../Rn" of 1 .. ULCX_MAX_RUNGS settings, each in parse_rate's syntax; returns the number of rungs, -1 for a
 * malformed one (an empty rung: "-50/", "/64", "-50//64"; too many; a rung parse_rate refuses) */
static int parse_ladder(const char *s, ulcx_rate *r, int *isAuto) {
    int n = 0;
    for (;;) {
        const char *slash = strchr(s, '/');
        const size_t len = slash ? (size_t)(slash - s) : strlen(s);
        char one[64];
        if (len == 0 || len >= sizeof(one) || n == ULCX_MAX_RUNGS) return -1;
        memcpy(one, s, len); one[len] = 0;
        if (parse_rate(one, &r[n], &isAuto[n])) return -1;
        n++;
        if (!slash) return n;
        s = slash + 1;
    }
}

/* The analysis pass over a batch of open inputs: each file's BlockComplexity summed over its own ceil(frames/BS)+2 blocks,
 * in block order, in double precision (ulcEncodeTool.c:93-98,130,164,178); nSwitched (may be NULL): its blocks whose
 * WindowCtrl is not the full-size, full-overlap 0x10.  Leaves the encoder's state behind the last block. */
static int analysis_pass(ulcx_encoder *enc, struct wav *w, int B, int bs, uint32_t maxBlk, float *pcm, void *tmp,
                         float *cplx, int32_t *wc, double *cplxSum, uint32_t *nSwitched) {
    const size_t frame = (size_t)bs * w[0].chan;
    for (uint32_t k0 = 0; k0 < maxBlk; k0 += KBLOCKS) {
        int K = (maxBlk - k0 < KBLOCKS) ? (int)(maxBlk - k0) : KBLOCKS;
        for (int s = 0; s < B; s++)
            wav_read(&w[s], k0 * (uint32_t)bs, (uint32_t)(K * bs), pcm + (size_t)s * K * frame, tmp);
        if (ulcx_analyse_host(enc, pcm, K, nSwitched ? wc : NULL, cplx) != ULCX_OK) DIE("analysis pass: %s", ulcx_last_error());
        for (int s = 0; s < B; s++) {
            uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
            for (int k = 0; k < K && k0 + (uint32_t)k < nb; k++) {
                cplxSum[s] += cplx[s * K + k];
                if (nSwitched && wc[s * K + k] != 0x10) nSwitched[s]++;
            }
        }
    }
    return 0;
}

static int analyse_group(const struct group *g) {
    const int bs = g->bs, B = g->n;
    struct wav *w = (struct wav *)calloc((size_t)B, sizeof(*w));
    uint32_t maxBlk = 0;
    for (int s = 0; s < B; s++) {
        int e = wav_open(&w[s], g->files[s]);
        if (e) DIE("cannot read '%s' (error %d: RIFF PCM16 / float32 only)", g->files[s], e);
        if (w[s].rate != w[0].rate || w[s].chan != w[0].chan) DIE("'%s': all inputs of one call must share rate and channel count", g->files[s]);
        uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;      /* ulcEncodeTool.c:93-98 */
        if (nb > maxBlk) maxBlk = nb;
    }
    const int C = w[0].chan;
    ulcx_encoder *enc = NULL;
    if (ulcx_encoder_create(&enc, g->device, B, C, bs, w[0].rate, KBLOCKS) != ULCX_OK) DIE("encoder: %s", ulcx_last_error());
    const size_t frame = (size_t)bs * C;
    float *pcm = (float *)malloc(sizeof(float) * (size_t)B * KBLOCKS * frame);
    float *cplx = (float *)malloc(sizeof(float) * (size_t)B * KBLOCKS);
    int32_t *wc = (int32_t *)malloc(sizeof(int32_t) * (size_t)B * KBLOCKS);
    double *cplxSum = (double *)calloc((size_t)B, sizeof(double));
    uint32_t *nSw = (uint32_t *)calloc((size_t)B, sizeof(uint32_t));
    void *tmp = malloc(frame * 4 * KBLOCKS);
    const int rc = analysis_pass(enc, w, B, bs, maxBlk, pcm, tmp, cplx, wc, cplxSum, nSw);
    for (int s = 0; s < B && !rc; s++) {
        uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
        /* (float): the value "RATE,auto" encodes with, and what `RATE,<complexity>` parses back */
        printf("%s: %u blocks, avg complexity %.9g, %u window-switched\n", base_name(g->files[s]), nb, (double)(float)(cplxSum[s] / nb), nSw[s]);
    }
    for (int s = 0; s < B; s++) fclose(w[s].f);
    ulcx_encoder_destroy(enc);
    free(pcm); free(cplx); free(wc); free(cplxSum); free(nSw); free(tmp); free(w);
    return rc;
}

static int encode_group(const struct group *g) {
    const char *outdir = g->outdir;
    const int bs = g->bs, B = g->n, a = 0, R = g->nRungs;
    char **argv = g->files;
    struct wav *w = (struct wav *)calloc((size_t)B, sizeof(*w));
    uint32_t maxBlk = 0;
    for (int s = 0; s < B; s++) {
        int e = wav_open(&w[s], argv[a + s]);
        if (e) DIE("cannot read '%s' (error %d: RIFF PCM16 / float32 only)", argv[a + s], e);
        if (w[s].rate != w[0].rate || w[s].chan != w[0].chan) DIE("'%s': all inputs of one call must share rate and channel count", argv[a + s]);
        uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;      /* ulcEncodeTool.c:93-98 */
        if (nb > maxBlk) maxBlk = nb;
    }
    const int C = w[0].chan, hz = w[0].rate;
    /* per rung: one setting for every file - the batch-wide form (ulcEncodeTool.c:157-159) -, otherwise the per-stream table */
    int uniform[ULCX_MAX_RUNGS], anyAuto = 0;
    for (int r = 0; r < R; r++) {
        uniform[r] = 1;
        for (int s = 0; s < B; s++) {
            const ulcx_rate *x = &g->setting[s * ULCX_MAX_RUNGS + r], *x0 = &g->setting[r];
            anyAuto |= g->autoc[s * ULCX_MAX_RUNGS + r];
            if (g->autoc[s * ULCX_MAX_RUNGS + r] || x->RateKbps != x0->RateKbps || x->AvgComplexity != x0->AvgComplexity) uniform[r] = 0;
        }
    }
    ulcx_rate *table = (ulcx_rate *)calloc((size_t)R * B, sizeof(ulcx_rate));         /* [R][B] */
    ulcx_encoder *enc = NULL;
    if (ulcx_encoder_create(&enc, g->device, B, C, bs, hz, KBLOCKS) != ULCX_OK) DIE("encoder: %s", ulcx_last_error());
    const int slot = ulcx_encoder_slot_bytes(enc);
    size_t frame = (size_t)bs * C;
    float *pcm = (float *)malloc(sizeof(float) * (size_t)B * KBLOCKS * frame);
    uint8_t *out = (uint8_t *)malloc((size_t)R * B * KBLOCKS * slot);                 /* [R][B][K][slot] */
    int32_t *bits = (int32_t *)malloc(sizeof(int32_t) * (size_t)R * B * KBLOCKS);     /* [R][B][K] */
    float *cplx = (float *)malloc(sizeof(float) * (size_t)B * KBLOCKS);
    double *cplxSum = (double *)calloc((size_t)B, sizeof(double));   /* ulcEncodeTool.c:130,164: feeds the ABR workflow */
    void *tmp = malloc(frame * 4 * KBLOCKS);
    FILE **fo = (FILE **)calloc((size_t)R * B, sizeof(FILE *));                       /* [R][B], as total and maxb */
    uint64_t *total = (uint64_t *)calloc((size_t)R * B, sizeof(uint64_t));
    uint32_t *maxb = (uint32_t *)calloc((size_t)R * B, sizeof(uint32_t));
    char path[1024];
    /* -index: one row per (rung, file) in the order of the call's output, grown after every encode call.  The decoder object
     * lends its geometry and tables only (one stream, one block per call). */
    const int nRows = R * B, iStride = (int)maxBlk + 1;
    ulcx_decoder *idec = NULL;
    ulcx_index_entry *idx = NULL; int32_t *idxN = NULL, *ibits = NULL;
    if (g->index) {
        if (ulcx_decoder_create(&idec, g->device, 1, C, bs, 1) != ULCX_OK) DIE("index: %s", ulcx_last_error());
        idx = (ulcx_index_entry *)malloc(sizeof(ulcx_index_entry) * (size_t)nRows * iStride);
        idxN = (int32_t *)calloc((size_t)nRows, sizeof(int32_t));
        ibits = (int32_t *)malloc(sizeof(int32_t) * (size_t)nRows * KBLOCKS);
        if (!idx || !idxN || !ibits) DIE("out of memory");
        for (size_t i = 0; i < (size_t)nRows * iStride; i++) {                       /* an open index, as ulcx_index_begin_dev leaves it */
            const int head = i % (size_t)iStride == 0;
            idx[i].ByteOffs = head ? 0 : -1; idx[i].RngState = head ? 1234567u : 0u;
        }
    }
    if (anyAuto) {
        /* "RATE,auto": pass 1 (analysis only: BlockComplexity does not depend on the rate mode, so every auto rung of a
         * ladder shares it) sums each file's complexity over its own blocks in block order in double precision
         * (ulcEncodeTool.c:130,164,178); after a reset, pass 2 encodes that file in ABR at (float)(sum / nBlocks) - in CBR if
         * that is 0, as the tool does with RATE,0 */
        const int rca = analysis_pass(enc, w, B, bs, maxBlk, pcm, tmp, cplx, NULL, cplxSum, NULL);
        if (rca) return rca;
        if (ulcx_encoder_reset(enc) != ULCX_OK) DIE("encoder reset: %s", ulcx_last_error());
    }
    for (int s = 0; s < B; s++) {
        for (int r = 0; r < R; r++) {
            table[r * B + s] = g->setting[s * ULCX_MAX_RUNGS + r];
            if (g->autoc[s * ULCX_MAX_RUNGS + r]) {
                uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
                table[r * B + s].AvgComplexity = (float)(cplxSum[s] / nb);
            }
        }
        cplxSum[s] = 0.0;                                              /* (pass 2 sums it again for the report) */
    }
    for (int s = 0; s < B; s++)
        for (int r = 0; r < R; r++) {
            char ext[32] = ".ulc";                                     /* a ladder: stem.r<i>.ulc */
            if (R > 1) snprintf(ext, sizeof(ext), ".r%d.ulc", r);
            out_path(path, sizeof(path), outdir, argv[a + s], ext);
            fo[r * B + s] = fopen(path, "wb");
            if (!fo[r * B + s]) DIE("cannot create '%s'", path);
            fseek(fo[r * B + s], 24, SEEK_SET);
        }
    /* a rung goes out as a scalar rung when all files share its setting, else as a table */
    ulcx_rung rungs[ULCX_MAX_RUNGS];
    memset(rungs, 0, sizeof(rungs));
    for (int r = 0; r < R; r++) {
        const float rate = table[r * B].RateKbps, avgc = table[r * B].AvgComplexity;
        rungs[r].mode = rate < 0.0f ? ULCX_MODE_VBR : (avgc > 0.0f ? ULCX_MODE_ABR : ULCX_MODE_CBR);
        rungs[r].param0 = rate < 0.0f ? -rate : rate; rungs[r].param1 = avgc;
        rungs[r].rate = uniform[r] ? NULL : table + (size_t)r * B;
    }
    for (uint32_t k0 = 0; k0 < maxBlk; k0 += KBLOCKS) {
        int K = (maxBlk - k0 < KBLOCKS) ? (int)(maxBlk - k0) : KBLOCKS;
        for (int s = 0; s < B; s++)
            wav_read(&w[s], k0 * (uint32_t)bs, (uint32_t)(K * bs), pcm + (size_t)s * K * frame, tmp);
        const int rc = R > 1 ? ulcx_encode_host_ladder(enc, rungs, R, pcm, K, out, bits, NULL, cplx)
                     : uniform[0] ? ulcx_encode_host(enc, rungs[0].mode, rungs[0].param0, rungs[0].param1, pcm, K, out, bits, NULL, cplx)
                                  : ulcx_encode_host_rates(enc, table, pcm, K, out, bits, NULL, cplx);
        if (rc != ULCX_OK) DIE("encode: %s", ulcx_last_error());
        for (int s = 0; s < B; s++) {
            uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
            for (int k = 0; k < K && k0 + (uint32_t)k < nb; k++) {
                for (int r = 0; r < R; r++) {
                    const size_t at = ((size_t)r * B + s) * K + k;
                    uint32_t sz = (uint32_t)(bits[at] + 7) / 8u;
                    fwrite(out + at * slot, 1, sz, fo[r * B + s]);                    /* ulcEncodeTool.c:160-169 */
                    total[r * B + s] += sz; if (sz > maxb[r * B + s]) maxb[r * B + s] = sz;
                }
                cplxSum[s] += cplx[s * K + k];
            }
        }
        if (g->index) {
            /* a file that has ended stops growing: size 0 from its last block on (the encoder goes on coding silence for it) */
            for (int r = 0; r < R; r++)
                for (int s = 0; s < B; s++) {
                    const uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
                    for (int k = 0; k < K; k++) { const size_t at = ((size_t)r * B + s) * K + k; ibits[at] = k0 + (uint32_t)k < nb ? bits[at] : 0; }
                }
            if (ulcx_index_slots_host(idec, nRows, out, slot, ibits, K, idx, iStride, idxN) != ULCX_OK) DIE("index: %s", ulcx_last_error());
        }
    }
    for (int s = 0; s < B; s++) {
        uint32_t nb = (w[s].nFrames + (uint32_t)bs - 1) / (uint32_t)bs + 2;
        if (R > 1) printf("%s: %u blocks, avg complexity %.5f", base_name(argv[a + s]), nb, cplxSum[s] / nb);
        for (int r = 0; r < R; r++) {
            const int i = r * B + s;
            ulcx_file_header h;
            h.Magic = ULCX_ULC_MAGIC; h.BlockSize = (uint16_t)bs; h.MaxBlockSize = (uint16_t)maxb[i]; h.nBlocks = nb;
            h.RateHz = (uint32_t)hz; h.nChan = (uint16_t)C; h.StreamOffs = 24;
            h.RateKbps = (uint16_t)ulcx_ulc_rate_kbps(total[i], (uint32_t)hz, (uint32_t)bs, nb);
            uint8_t hb[24]; ulcx_ulc_header_pack(hb, &h);
            fseek(fo[i], 0, SEEK_SET); fwrite(hb, 1, 24, fo[i]); fclose(fo[i]);
            if (g->index) {
                char ext[32] = ".ulx";
                if (R > 1) snprintf(ext, sizeof(ext), ".r%d.ulx", r);
                out_path(path, sizeof(path), outdir, argv[a + s], ext);
                FILE *fx = fopen(path, "wb");
                if (!fx) DIE("cannot create '%s'", path);
                if ((uint32_t)idxN[i] != nb) fprintf(stderr, "ulcx-tool: %s: %d of %u blocks indexed\n", path, (int)idxN[i], nb);
                ulcx_index_file_header xh;
                xh.Magic = ULCX_ULX_MAGIC; xh.BlockSize = (uint16_t)bs; xh.nChan = (uint16_t)C; xh.nBlocks = (uint32_t)idxN[i]; xh.PayloadBytes = (uint32_t)total[i];
                uint8_t xb[ULCX_ULX_HEADER_BYTES]; ulcx_ulx_header_pack(xb, &xh);
                fwrite(xb, 1, sizeof(xb), fx);
                for (int k = 0; k <= idxN[i]; k++) {                                   /* little-endian, whatever the host is */
                    const ulcx_index_entry *en = &idx[(size_t)i * iStride + k];
                    const uint32_t o = (uint32_t)en->ByteOffs, st = en->RngState;
                    const uint8_t eb[8] = { (uint8_t)o, (uint8_t)(o >> 8), (uint8_t)(o >> 16), (uint8_t)(o >> 24), (uint8_t)st, (uint8_t)(st >> 8), (uint8_t)(st >> 16), (uint8_t)(st >> 24) };
                    fwrite(eb, 1, 8, fx);
                }
                fclose(fx);
            }
            char used[64] = "";                                                        /* "RATE,auto": the complexity pass 2 used */
            if (g->autoc[s * ULCX_MAX_RUNGS + r]) snprintf(used, sizeof(used), "ABR complexity %.9g%s", (double)table[i].AvgComplexity, table[i].AvgComplexity > 0.0f ? "" : " (CBR)");
            if (R > 1) printf("; r%d: %.2f KiB, %u kbps%s%s", r, total[i] / 1024.0, h.RateKbps, used[0] ? ", " : "", used);
            else printf("%s: %u blocks, %.2f KiB, %u kbps, %s%savg complexity %.5f\n", base_name(argv[a + s]), nb, total[i] / 1024.0, h.RateKbps,
                        used, used[0] ? ", " : "", cplxSum[s] / nb);                  /* ulcEncodeTool.c:176,186 */
        }
        if (R > 1) printf("\n");
        fclose(w[s].f);
    }
    ulcx_encoder_destroy(enc);
    if (idec) ulcx_decoder_destroy(idec);
    free(idx); free(idxN); free(ibits);
    free(pcm); free(out); free(bits); free(cplx); free(cplxSum); free(tmp); free(fo); free(total); free(maxb); free(w); free(table);
    return 0;
}

/* The `.ulx` beside a `.ulc` input: its entries (caller frees) when the header agrees with the container's and the index
 * passes ulcx_index_check against the payload's size; NULL and a reason otherwise. */
static ulcx_index_entry *load_sidecar(const char *ulcPath, const ulcx_file_header *h, int32_t payBytes, const char **why) {
    char path[1024];
    const size_t n = strlen(ulcPath);
    *why = "no .ulx beside it";
    if (n < 4 || n + 1 > sizeof(path) || strcmp(ulcPath + n - 4, ".ulc")) return NULL;
    memcpy(path, ulcPath, n + 1); path[n - 1] = 'x';
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    uint8_t hb[ULCX_ULX_HEADER_BYTES];
    ulcx_index_file_header xh;
    ulcx_index_entry *ent = NULL;
    *why = "its .ulx is short or not a block index";
    if (fread(hb, 1, sizeof(hb), f) == sizeof(hb) && ulcx_ulx_header_parse(&xh, hb, sizeof(hb)) == ULCX_OK) {
        *why = "its .ulx was made for another file (header mismatch)";
        if (xh.BlockSize == h->BlockSize && xh.nChan == h->nChan && xh.nBlocks == h->nBlocks && xh.PayloadBytes == (uint32_t)payBytes) {
            const size_t cnt = (size_t)xh.nBlocks + 1;
            uint8_t *raw = (uint8_t *)malloc(cnt * 8);
            ent = (ulcx_index_entry *)malloc(cnt * sizeof(*ent));
            *why = "its .ulx is short or not a block index";
            if (raw && ent && fread(raw, 8, cnt, f) == cnt) {
                for (size_t k = 0; k < cnt; k++) { ent[k].ByteOffs = (int32_t)rd32(raw + 8 * k); ent[k].RngState = rd32(raw + 8 * k + 4); }
                *why = "its .ulx does not pass ulcx_index_check";
                if (ulcx_index_check(ent, (int)xh.nBlocks, (int)cnt, payBytes) != ULCX_OK) { free(ent); ent = NULL; }
            } else { free(ent); ent = NULL; }
            free(raw);
        }
    }
    fclose(f);
    return ent;
}

static int decode_group(const struct group *g) {
    const char *outdir = g->outdir;
    const int isFloat = g->isFloat, B = g->n, a = 0;
    char **argv = g->files;
    ulcx_file_header *h = (ulcx_file_header *)calloc((size_t)B, sizeof(*h));
    uint8_t **pay = (uint8_t **)calloc((size_t)B, sizeof(uint8_t *));
    int32_t *payBytes = (int32_t *)calloc((size_t)B, sizeof(int32_t));
    long long stride = 0;
    uint32_t maxBlk = 0;
    for (int s = 0; s < B; s++) {
        FILE *f = fopen(argv[a + s], "rb");
        if (!f) DIE("cannot open '%s'", argv[a + s]);
        fseek(f, 0, SEEK_END); long len = ftell(f); fseek(f, 0, SEEK_SET);
        uint8_t *buf = (uint8_t *)malloc((size_t)len + 16);
        if (fread(buf, 1, (size_t)len, f) != (size_t)len) DIE("short read on '%s'", argv[a + s]);
        fclose(f);
        if (ulcx_ulc_header_parse(&h[s], buf, (size_t)len)) DIE("'%s' is not a ULC2 container", argv[a + s]);
        /* the header is untrusted input: validate it before anything is sized or indexed from it */
        if (h[s].StreamOffs < 24 || (long)h[s].StreamOffs > len) DIE("'%s': stream offset %u outside the file (%ld bytes)", argv[a + s], h[s].StreamOffs, len);
        if (h[s].nChan < 1 || h[s].nChan > 255 || h[s].BlockSize < 256 || h[s].BlockSize > 32768 || (h[s].BlockSize & (h[s].BlockSize - 1)))
            DIE("'%s': invalid geometry in the header (BlockSize %u, %u channels)", argv[a + s], h[s].BlockSize, h[s].nChan);
        if (h[s].BlockSize != h[0].BlockSize || h[s].nChan != h[0].nChan || h[s].RateHz != h[0].RateHz)
            DIE("'%s': all inputs of one call must share block size, channels and rate", argv[a + s]);
        /* block count and payload size too: a block is at least two bytes (window nybble + one code per channel), so a
         * header that counts more blocks than the payload can hold is corrupt, and so is a payload the 32-bit read
         * positions of the library cannot address; the WAV header's sample count is checked in 64 bits */
        if (len - (long)h[s].StreamOffs > 0x7fffffffL) DIE("'%s': payload of %ld bytes is more than this tool takes (2 GiB)", argv[a + s], len - (long)h[s].StreamOffs);
        if ((uint64_t)h[s].nBlocks > (uint64_t)(len - (long)h[s].StreamOffs) / 2) DIE("'%s': header counts %u blocks, the payload has %ld bytes", argv[a + s], h[s].nBlocks, len - (long)h[s].StreamOffs);
        if ((uint64_t)h[s].nBlocks * h[s].BlockSize * h[s].nChan * 4 > 0xfffff000ull) DIE("'%s': %u blocks decode to more than a WAV file holds", argv[a + s], h[s].nBlocks);
        pay[s] = buf; payBytes[s] = (int32_t)(len - (long)h[s].StreamOffs);
        if (payBytes[s] + 8 > stride) stride = payBytes[s] + 8;
        if (h[s].nBlocks > maxBlk) maxBlk = h[s].nBlocks;
    }
    const int bs = h[0].BlockSize, C = h[0].nChan;
    /* -blocks:FIRST,COUNT: nOut[s] blocks of file s from block FIRST on; else the whole file */
    const int range = g->rCount > 0;
    uint32_t *nOut = (uint32_t *)calloc((size_t)B, sizeof(uint32_t));
    int32_t *first = (int32_t *)calloc((size_t)B, sizeof(int32_t));
    uint32_t total = maxBlk;
    if (range) {
        total = 0;
        for (int s = 0; s < B; s++) {
            if ((uint32_t)g->rFirst >= h[s].nBlocks) DIE("'%s': -blocks starts at block %d, the file has %u blocks", argv[a + s], (int)g->rFirst, h[s].nBlocks);
            const uint32_t left = h[s].nBlocks - (uint32_t)g->rFirst;
            nOut[s] = left < (uint32_t)g->rCount ? left : (uint32_t)g->rCount;
            if (nOut[s] > total) total = nOut[s];
        }
    } else for (int s = 0; s < B; s++) nOut[s] = h[s].nBlocks;
    stride = (stride + 15) & ~15LL;
    uint8_t *payload = (uint8_t *)calloc((size_t)B, (size_t)stride);
    for (int s = 0; s < B; s++) { memcpy(payload + (size_t)s * stride, pay[s] + h[s].StreamOffs, (size_t)payBytes[s]); free(pay[s]); }
    ulcx_decoder *dec = NULL;
    if (ulcx_decoder_create(&dec, g->device, B, C, bs, KBLOCKS) != ULCX_OK) DIE("decoder: %s", ulcx_last_error());
    size_t frame = (size_t)bs * C;
    float *pcm = (float *)malloc(sizeof(float) * (size_t)B * KBLOCKS * frame);
    int32_t *bits = (int32_t *)malloc(sizeof(int32_t) * (size_t)B * KBLOCKS);
    int16_t *tmp = (int16_t *)malloc(sizeof(int16_t) * frame);
    FILE **fo = (FILE **)calloc((size_t)B, sizeof(FILE *));
    char path[1024];
    for (int s = 0; s < B; s++) {
        out_path(path, sizeof(path), outdir, argv[a + s], ".wav");
        fo[s] = fopen(path, "wb");
        if (!fo[s]) DIE("cannot create '%s'", path);
        wav_write_header(fo[s], (int)h[s].RateHz, C, isFloat, nOut[s] * (uint32_t)bs);
    }
    if (ulcx_decoder_upload_payload(dec, payload, stride, payBytes) != ULCX_OK) DIE("upload: %s", ulcx_last_error());   /* once, not per call */
    int rcAll = 0;
    /* (a range call runs the block in front of its range too: one block fewer per call) */
    const uint32_t step = range ? KBLOCKS - 1 : KBLOCKS, blk0 = range ? (uint32_t)g->rFirst : 0;
    if (range) {
        /* stored indexes when every input has a usable one, else the walk (once) */
        ulcx_index_entry **side = (ulcx_index_entry **)calloc((size_t)B, sizeof(*side));
        int have = 1;
        for (int s = 0; s < B && have; s++) {
            const char *why = "";
            side[s] = load_sidecar(argv[a + s], &h[s], payBytes[s], &why);
            if (!side[s]) { fprintf(stderr, "ulcx-tool: %s: %s: indexing the payloads\n", argv[a + s], why); have = 0; }
        }
        if (have) {
            const int iStride = (int)maxBlk + 1;
            ulcx_index_entry *rows = (ulcx_index_entry *)malloc(sizeof(*rows) * (size_t)B * iStride);
            int32_t *cnt = (int32_t *)malloc(sizeof(int32_t) * (size_t)B);
            if (!rows || !cnt) DIE("out of memory");
            for (int s = 0; s < B; s++) {
                cnt[s] = (int32_t)h[s].nBlocks;
                for (int k = 0; k < iStride; k++) {
                    ulcx_index_entry *e = &rows[(size_t)s * iStride + k];
                    if ((uint32_t)k <= h[s].nBlocks) *e = side[s][k]; else { e->ByteOffs = -1; e->RngState = 0u; }
                }
            }
            if (ulcx_decoder_set_resident_index(dec, rows, iStride, cnt) != ULCX_OK) {
                fprintf(stderr, "ulcx-tool: stored block index refused (%s): indexing the payloads\n", ulcx_last_error());
                have = 0;
            }
            free(rows); free(cnt);
        }
        for (int s = 0; s < B; s++) free(side[s]);
        free(side);
        if (!have && ulcx_decoder_index_resident(dec, (int)(blk0 + total), NULL) != ULCX_OK) DIE("index: %s", ulcx_last_error());
    }
    for (uint32_t k0 = 0; k0 < total; k0 += step) {
        int K = (total - k0 < step) ? (int)(total - k0) : (int)step;
        if (range) {
            for (int s = 0; s < B; s++) first[s] = (int32_t)(blk0 + k0);
            if (ulcx_decode_resident_range_host(dec, first, K, pcm, bits) != ULCX_OK) DIE("decode: %s", ulcx_last_error());
        } else if (ulcx_decode_resident_host(dec, K, pcm, bits) != ULCX_OK) DIE("decode: %s", ulcx_last_error());
        for (int s = 0; s < B; s++)
            for (int k = 0; k < K && k0 + (uint32_t)k < nOut[s]; k++) {
                if (!bits[s * K + k]) { fprintf(stderr, "ulcx-tool: %s: corrupted stream at block %u\n", argv[a + s], blk0 + k0 + (uint32_t)k); rcAll = 1; }
                const float *src = pcm + ((size_t)s * K + k) * frame;
                if (isFloat) fwrite(src, 4, frame, fo[s]);
                else {
                    for (size_t i = 0; i < frame; i++) {                                  /* WavIO_Helper.c:57-63 */
                        float v = src[i] * 0x1.0p+15f;
                        v = v < -32768.0f ? -32768.0f : (v > 32767.0f ? 32767.0f : v);
                        tmp[i] = (int16_t)lrintf(v);
                    }
                    fwrite(tmp, 2, frame, fo[s]);
                }
            }
    }
    for (int s = 0; s < B; s++) fclose(fo[s]);
    ulcx_decoder_destroy(dec);
    free(payload); free(pcm); free(bits); free(tmp); free(fo); free(h); free(pay); free(payBytes); free(nOut); free(first);
    return rcAll;
}

static void *group_main(void *p) {
    struct group *g = (struct group *)p;
    g->rc = g->decode ? decode_group(g) : g->analyse ? analyse_group(g) : encode_group(g);
    return NULL;
}
/* the command line's inputs as nDev groups (input i goes to group i % nDev), one host thread and one codec object each */
static int run_groups(struct group *proto, int nFiles, char **files, int nDev) {
    if (nFiles < 1) DIE("no input files");
    if (nDev > nFiles) nDev = nFiles;
    const int have = ulcx_device_count();
    if (have < 1) DIE("no HIP device: %s", ulcx_last_error());
    if (nDev <= 1) { proto->device = 0; proto->n = nFiles; proto->files = files; return proto->decode ? decode_group(proto) : proto->analyse ? analyse_group(proto) : encode_group(proto); }
    /* what a single group checks per batch - every input of one call shares rate / channels (encode) or block size /
     * channels / rate (decode) - is checked here ONCE over all files, before they are dealt out: a command line that a
     * one-group run rejects must not be partly accepted with -devices:N */
    {
        uint32_t ref[3] = { 0, 0, 0 };
        for (int i = 0; i < nFiles; i++) {
            uint32_t cur[3] = { 0, 0, 0 };
            if (!proto->decode) {
                struct wav w;
                const int e = wav_open(&w, files[i]);
                if (e) DIE("cannot read '%s' (error %d: RIFF PCM16 / float32 only)", files[i], e);
                cur[0] = w.rate; cur[1] = (uint32_t)w.chan; fclose(w.f);
            } else {
                uint8_t hb[24]; ulcx_file_header h;
                FILE *f = fopen(files[i], "rb");
                if (!f) DIE("cannot open '%s'", files[i]);
                const size_t got = fread(hb, 1, sizeof(hb), f); fclose(f);
                if (got != sizeof(hb) || ulcx_ulc_header_parse(&h, hb, sizeof(hb))) DIE("'%s' is not a ULC2 container", files[i]);
                cur[0] = h.RateHz; cur[1] = h.nChan; cur[2] = h.BlockSize;
            }
            if (i == 0) memcpy(ref, cur, sizeof(ref));
            else if (memcmp(ref, cur, sizeof(ref))) DIE("'%s': all inputs of one call must share %s", files[i], proto->decode ? "block size, channels and rate" : "rate and channel count");
        }
    }
    struct group *gs = (struct group *)calloc((size_t)nDev, sizeof(*gs));
    char **deal = (char **)calloc((size_t)nFiles, sizeof(char *));
    ulcx_rate *dealR = (ulcx_rate *)calloc((size_t)nFiles * ULCX_MAX_RUNGS, sizeof(ulcx_rate));     /* each file keeps its own settings */
    int *dealA = (int *)calloc((size_t)nFiles * ULCX_MAX_RUNGS, sizeof(int));
    pthread_t *th = (pthread_t *)calloc((size_t)nDev, sizeof(pthread_t));
    if (!gs || !deal || !dealR || !dealA || !th) { free(gs); free(deal); free(dealR); free(dealA); free(th); DIE("out of memory"); }
    int at = 0, rc = 0, started = 0;
    for (int g = 0; g < nDev; g++) {
        gs[g] = *proto; gs[g].device = g % have; gs[g].files = deal + at; gs[g].setting = dealR + (size_t)at * ULCX_MAX_RUNGS; gs[g].autoc = dealA + (size_t)at * ULCX_MAX_RUNGS; gs[g].n = 0; gs[g].rc = 0;
        for (int i = g; i < nFiles; i += nDev) {
            if (!proto->decode && !proto->analyse) {
                memcpy(dealR + (size_t)(at + gs[g].n) * ULCX_MAX_RUNGS, proto->setting + (size_t)i * ULCX_MAX_RUNGS, sizeof(ulcx_rate) * ULCX_MAX_RUNGS);
                memcpy(dealA + (size_t)(at + gs[g].n) * ULCX_MAX_RUNGS, proto->autoc + (size_t)i * ULCX_MAX_RUNGS, sizeof(int) * ULCX_MAX_RUNGS);
            }
            deal[at + gs[g].n++] = files[i];
        }
        at += gs[g].n;
    }
    for (int g = 0; g < nDev; g++) {
        if (pthread_create(&th[g], NULL, group_main, &gs[g])) { fprintf(stderr, "ulcx-tool: cannot start a host thread for group %d\n", g); rc = 2; break; }
        started++;
    }
    /* (a failed start: the groups already running work on gs / deal - they are joined before anything is freed) */
    for (int g = 0; g < started; g++) { pthread_join(th[g], NULL); if (gs[g].rc > rc) rc = gs[g].rc; }
    free(gs); free(deal); free(dealR); free(dealA); free(th);
    return rc;
}
/* "-rate:LADDER": the setting of the inputs that follow; every group of one command names as many rungs as RATE does */
static int parse_rate_group(const char *arg, ulcx_rate *cur, int *curAuto, int nRungs) {
    ulcx_rate r[ULCX_MAX_RUNGS]; int au[ULCX_MAX_RUNGS];
    const int n = parse_ladder(arg + 6, r, au);
    if (n < 0) DIE("invalid coding rate '%s'", arg);
    if (n != nRungs) DIE("'%s' names %d rung%s, RATE names %d: every -rate: group of one command needs as many rungs as RATE", arg, n, n == 1 ? "" : "s", nRungs);
    memcpy(cur, r, sizeof(r)); memcpy(curAuto, au, sizeof(au));
    return 0;
}
static int do_encode(int argc, char **argv) {
    if (argc < 5) DIE("usage: ulcx-tool encode OUTDIR RATE[,AvgComplexity|,auto][/RATE...] [-blocksize:N] [-devices:N] [-index] IN.wav [-rate:RATE[,...][/RATE...]] IN.wav ...");
    struct group g; memset(&g, 0, sizeof(g));
    g.outdir = argv[2];
    ulcx_rate cur[ULCX_MAX_RUNGS]; int curAuto[ULCX_MAX_RUNGS];
    memset(cur, 0, sizeof(cur)); memset(curAuto, 0, sizeof(curAuto));
    g.nRungs = parse_ladder(argv[3], cur, curAuto);
    if (g.nRungs < 0) DIE("invalid coding rate '%s' (RATE[,AvgComplexity|,auto], or a ladder R0/R1/... of 1 to %d of them)", argv[3], ULCX_MAX_RUNGS);
    int a = 4, nDev = 1, endOpts = 0;
    g.bs = 2048;
    for (; a < argc && argv[a][0] == '-'; a++) {
        if (!strcmp(argv[a], "--")) { a++; endOpts = 1; break; }    /* end of options: input names may start with '-' behind it */
        if (!strncmp(argv[a], "-blocksize:", 11)) g.bs = atoi(argv[a] + 11);
        else if (!strncmp(argv[a], "-devices:", 9)) nDev = atoi(argv[a] + 9);
        else if (!strcmp(argv[a], "-index")) g.index = 1;
        else if (!strncmp(argv[a], "-rate:", 6)) { if (parse_rate_group(argv[a], cur, curAuto, g.nRungs)) return 2; }
        else DIE("unknown option '%s'", argv[a]);
    }
    if (g.bs < 256 || g.bs > 8192 || (g.bs & -g.bs) != g.bs) DIE("unsupported block size %d", g.bs);
    if (nDev < 1 || nDev > 64) DIE("-devices:%d out of range", nDev);
    /* the inputs, each with the setting in force where it stands: "-rate:RATE[,AvgComplexity|,auto][/...]" between them sets it
     * for the inputs that follow (behind "--" every argument is an input) */
    char **files = (char **)calloc((size_t)(argc - a + 1), sizeof(char *));
    g.setting = (ulcx_rate *)calloc((size_t)(argc - a + 1) * ULCX_MAX_RUNGS, sizeof(ulcx_rate));
    g.autoc = (int *)calloc((size_t)(argc - a + 1) * ULCX_MAX_RUNGS, sizeof(int));
    if (!files || !g.setting || !g.autoc) DIE("out of memory");
    int n = 0;
    for (; a < argc; a++) {
        if (!endOpts && !strncmp(argv[a], "-rate:", 6)) { if (parse_rate_group(argv[a], cur, curAuto, g.nRungs)) return 2; continue; }
        files[n] = argv[a];
        memcpy(g.setting + (size_t)n * ULCX_MAX_RUNGS, cur, sizeof(cur)); memcpy(g.autoc + (size_t)n * ULCX_MAX_RUNGS, curAuto, sizeof(curAuto));
        n++;
    }
    const int rc = run_groups(&g, n, files, nDev);
    free(files); free(g.setting); free(g.autoc);
    return rc;
}
static int do_analyse(int argc, char **argv) {
    if (argc < 3) DIE("usage: ulcx-tool analyse [-blocksize:N] [-devices:N] IN.wav ...");
    struct group g; memset(&g, 0, sizeof(g));
    g.analyse = 1; g.bs = 2048;
    int a = 2, nDev = 1;
    for (; a < argc && argv[a][0] == '-'; a++) {
        if (!strcmp(argv[a], "--")) { a++; break; }
        if (!strncmp(argv[a], "-blocksize:", 11)) g.bs = atoi(argv[a] + 11);
        else if (!strncmp(argv[a], "-devices:", 9)) nDev = atoi(argv[a] + 9);
        else DIE("unknown option '%s'", argv[a]);
    }
    if (g.bs < 256 || g.bs > 8192 || (g.bs & -g.bs) != g.bs) DIE("unsupported block size %d", g.bs);
    if (nDev < 1 || nDev > 64) DIE("-devices:%d out of range", nDev);
    return run_groups(&g, argc - a, argv + a, nDev);
}
static int do_decode(int argc, char **argv) {
    if (argc < 4) DIE("usage: ulcx-tool decode OUTDIR [-format:PCM16|FLOAT32] [-blocks:FIRST,COUNT] [-devices:N] IN.ulc ...");
    struct group g; memset(&g, 0, sizeof(g));
    g.decode = 1; g.outdir = argv[2];
    int a = 3, nDev = 1;
    for (; a < argc && argv[a][0] == '-'; a++) {
        if (!strcmp(argv[a], "--")) { a++; break; }
        if (!strncmp(argv[a], "-format:", 8)) {
            const char *f = argv[a] + 8;
            if (!strcmp(f, "FLOAT32") || !strcmp(f, "float32")) g.isFloat = 1;
            else if (strcmp(f, "PCM16") && strcmp(f, "pcm16")) DIE("unsupported output format '%s'", f);
        } else if (!strncmp(argv[a], "-devices:", 9)) nDev = atoi(argv[a] + 9);
        else if (!strncmp(argv[a], "-blocks:", 8)) {
            /* FIRST >= 0, COUNT >= 1, both plain decimal numbers; FIRST + COUNT within the container's 32-bit block count */
            char *e1 = NULL, *e2 = NULL;
            const char *v = argv[a] + 8;
            const long long f = strtoll(v, &e1, 10);
            const long long n = (e1 != v && *e1 == ',') ? strtoll(e1 + 1, &e2, 10) : 0;
            if (e1 == v || *e1 != ',' || e2 == e1 + 1 || *e2 || v[0] == '+' || e1[1] == '+' || f < 0 || n < 1 || f > 0x3fffffffLL || n > 0x3fffffffLL)
                DIE("invalid block range '%s' (-blocks:FIRST,COUNT with FIRST >= 0, COUNT >= 1)", argv[a]);
            g.rFirst = (int32_t)f; g.rCount = (int32_t)n;
        } else DIE("unknown option '%s'", argv[a]);
    }
    if (nDev < 1 || nDev > 64) DIE("-devices:%d out of range", nDev);
    return run_groups(&g, argc - a, argv + a, nDev);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "encode")) return do_encode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "decode")) return do_decode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "analyse")) return do_analyse(argc, argv);
    fprintf(stderr,
            "ulcx-tool - batched ulc-codec front-end over libulc_amd.so (MI355X)\n"
            "  ulcx-tool encode OUTDIR RATE[,AvgComplexity] [-blocksize:N] [-devices:N] [-index] IN1.wav [-rate:RATE[,...]] IN2.wav ...\n"
            "      RATE < 0: VBR quality; RATE > 0: CBR kbps; RATE,AvgComplexity: ABR  (as ulcencodetool)\n"
            "      RATE,auto: two-pass ABR at each file's own average complexity (0: CBR)\n"
            "      -rate:RATE[,AvgComplexity|,auto]  setting of the inputs that follow it (RATE is the default)\n"
            "      -index  write a block index OUTDIR/stem.ulx (stem.r<i>.ulx) beside every file, grown from the encoder's output\n"
            "      R0/R1/.../Rn (RATE and every -rate:, the same count): a ladder, one OUTDIR/stem.r<i>.ulc per rung from one call\n"
            "  ulcx-tool decode OUTDIR [-format:PCM16|FLOAT32] [-blocks:FIRST,COUNT] [-devices:N] IN1.ulc IN2.ulc ...\n"
            "      -blocks:FIRST,COUNT  only blocks FIRST .. FIRST+COUNT-1 of every file (block index + range decode; IN.ulx is used when present)\n"
            "  ulcx-tool analyse [-blocksize:N] [-devices:N] IN1.wav IN2.wav ...\n"
            "      per file: blocks, the average complexity to feed RATE,<complexity> with, window-switched blocks; writes no file\n"
            "  --          end of options (input names that start with '-')\n"
            "  -devices:N  inputs dealt round-robin over N groups, one host thread + one codec object each (device g %% visible)\n");
    return 1;
}
