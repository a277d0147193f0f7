/*
 * ulc_ref_driver — TEST INFRASTRUCTURE ONLY (see oracle/README.md).  Written by this project.
 *
 * A command-line driver over the reference's public libulc API (ulcEncoder.h / ulcDecoder.h), linked against
 * _ref/libulc_ref_full.so: the seven reference sources compiled in place over standin/Fourier.h.  One run handles one
 * stream, so every stream starts from what a fresh tool run sees - fresh encoder state and the decoder's function-static
 * noise seed at its initial value.  Both directions take and give interleaved PCM, as the reference's tools do (the
 * "arranged sequentially" notes in ulcEncoder.h / ulcDecoder.h do not match the code, which reads and writes
 * Data[n*nChan+Chan]).
 *
 *   ulc_ref_driver enc IN.f32 OUT.bin BlockSize nChan RateHz mode p0 p1 nBlocks slot
 *       IN: nBlocks*BlockSize frames of interleaved float32 PCM.  mode 0 = VBR(p0 = quality), 1 = CBR(p0 = kbps),
 *       2 = ABR(p0 = kbps, p1 = AvgComplexity).  OUT: nBlocks records of
 *         int32 SizeBits, int32 WindowCtrl, int32 NextWindowCtrl, float32 BlockComplexity, uint8 bytes[slot]
 *       (the state fields as ULC_EncoderState_t holds them after the call; bytes zero-padded past (SizeBits+7)/8).
 *   ulc_ref_driver dec IN.bin OUT.bin BlockSize nChan nBlocks slot
 *       IN: nBlocks blocks of `slot` bytes.  OUT: int32 BitsRead[nBlocks], then nBlocks*BlockSize frames of interleaved
 *       float32 PCM.
 * Exit status 0 on success, 2 on bad arguments or I/O, 3 when a state fails to initialise or a block overflows its slot.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ulcEncoder.h"
#include "ulcDecoder.h"

static void *read_all(const char *path, size_t want) {
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    void *p = malloc(want ? want : 1);
    size_t got = p ? fread(p, 1, want, f) : 0;
    fclose(f);
    if (got != want) { free(p); return NULL; }
    return p;
}

static int encode(char **a) {
    int BS = atoi(a[2]), C = atoi(a[3]), rate = atoi(a[4]), mode = atoi(a[5]);
    float p0 = strtof(a[6], NULL), p1 = strtof(a[7], NULL);
    int nBlk = atoi(a[8]), slot = atoi(a[9]);
    if (BS <= 0 || C <= 0 || nBlk <= 0 || slot <= 0 || mode < 0 || mode > 2) return 2;
    size_t blk = (size_t)BS * C;
    float *pcm = read_all(a[0], sizeof(float) * blk * nBlk);
    if (!pcm) return 2;
    FILE *out = fopen(a[1], "wb");
    if (!out) return 2;
    struct ULC_EncoderState_t st;
    memset(&st, 0, sizeof(st));
    st.RateHz = rate; st.nChan = C; st.BlockSize = BS;
    if (ULC_EncoderState_Init(&st) < 0) return 3;
    uint8_t *rec = malloc(16 + (size_t)slot);
    int rc = 0;
    for (int k = 0; k < nBlk && !rc; k++) {
        const float *src = pcm + k * blk;
        int size = 0;
        const void *data;
        if (mode == 0) data = ULC_EncodeBlock_VBR(&st, src, &size, p0);
        else if (mode == 1) data = ULC_EncodeBlock_CBR(&st, src, &size, p0);
        else data = ULC_EncodeBlock_ABR(&st, src, &size, p0, p1);
        int nb = (size + 7) / 8;
        if (nb > slot) { rc = 3; break; }
        int32_t hdr[3] = { size, st.WindowCtrl, st.NextWindowCtrl };
        memcpy(rec, hdr, 12);
        memcpy(rec + 12, &st.BlockComplexity, 4);
        memset(rec + 16, 0, slot);
        memcpy(rec + 16, data, nb);
        if (fwrite(rec, 1, 16 + (size_t)slot, out) != 16 + (size_t)slot) rc = 2;
    }
    ULC_EncoderState_Destroy(&st);
    if (fclose(out)) rc = rc ? rc : 2;
    free(rec); free(pcm);
    return rc;
}

static int decode(char **a) {
    int BS = atoi(a[2]), C = atoi(a[3]), nBlk = atoi(a[4]), slot = atoi(a[5]);
    if (BS <= 0 || C <= 0 || nBlk <= 0 || slot <= 0) return 2;
    size_t blk = (size_t)BS * C;
    uint8_t *in = read_all(a[0], (size_t)slot * nBlk);
    if (!in) return 2;
    struct ULC_DecoderState_t st;
    memset(&st, 0, sizeof(st));
    st.nChan = C; st.BlockSize = BS;
    if (ULC_DecoderState_Init(&st) < 0) return 3;
    int32_t *bits = malloc(sizeof(int32_t) * nBlk);
    float *pcm = malloc(sizeof(float) * blk * nBlk);
    for (int k = 0; k < nBlk; k++) bits[k] = ULC_DecodeBlock(&st, pcm + k * blk, in + (size_t)k * slot);
    ULC_DecoderState_Destroy(&st);
    int rc = 0;
    FILE *out = fopen(a[1], "wb");
    if (!out) rc = 2;
    else {
        if (fwrite(bits, sizeof(int32_t), nBlk, out) != (size_t)nBlk || fwrite(pcm, sizeof(float), blk * nBlk, out) != blk * nBlk) rc = 2;
        if (fclose(out)) rc = 2;
    }
    free(pcm); free(bits); free(in);
    return rc;
}

int main(int argc, char **argv) {
    if (argc == 12 && !strcmp(argv[1], "enc")) return encode(argv + 2);
    if (argc == 8 && !strcmp(argv[1], "dec")) return decode(argv + 2);
    fprintf(stderr, "usage: %s enc IN.f32 OUT.bin BlockSize nChan RateHz mode p0 p1 nBlocks slot\n"
                    "       %s dec IN.bin OUT.bin BlockSize nChan nBlocks slot\n", argv[0], argv[0]);
    return 2;
}
