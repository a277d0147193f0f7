/* ulc_amd_lowrate.h — low-rate sample crops: 1/2, 1/4, 1/8 of the file's sample rate straight from the synthesis.
 *
 * A loader that trains at 24 or 16 kHz from a 48 kHz corpus need not decode at 48 kHz and resample.  The leading S / D coefficients
 * of every (sub-)block, run through the inverse transform of size S / D, ARE the signal band-limited to fs / 2D and sampled at
 * fs / D: a 1/D transform and 1/D of the output bytes, and no pass over the output.  These entries are the sample-crop calls of
 * ulc_amd.h (ulcx_decode_crops_samples_*) with one further argument, int lgD, behind nSamples; D = 1 << lgD, BS' = BlockSize / D.
 *
 *   ROWS      Row i is nSamples samples from sample d_start[i] (int64) of the REDUCED stream of file d_file[i]: sample j of that
 *             stream is sample j % BS' of block j / BS' - a reduced block is BS' samples of the same block of the file.  The row's
 *             leading d_len[i] samples (NULL: nSamples) are written, d_pcm [n][nChan][nSamples] in full: zeros behind the length,
 *             behind the file's last indexed block, and from a corrupt block on.
 *   A LIVE SAMPLE is, bit for bit, what the reference decoder of BlockSize BS' writes when, for every sub-block of size S / D, its
 *             TransformBuffer holds the leading S / D of the S coefficients the full decoder holds for that sub-block.  The noise
 *             fill is included: the generator draws for all S coefficients, so the noise in the shared bins is the full decode's.
 *             The window code is the block's own; the overlap is (S / D) >> scale, clipped to the previous sub-block's reduced
 *             size.  Mid/side un-mix and the PCM16 conversion are the sample-crop calls'.  Equivalently: ulcx_decode_crops_spectra_dev,
 *             the low bins of every sub-block (ulcx_window_subblocks), then ulcx_synth_spectra_dev with ULCX_SYNTH_WARM on a decoder
 *             of BlockSize BS'.  No coefficient plane exists in memory on the way.
 *   TIME      Reduced sample m sits at full-rate time D m + (D - 1) / 2 of the file's decoded stream, gain 1; the codec's delay is
 *             not compensated ("Low-rate crops").  The band edge is a sine-window MDCT's, not a brick wall:
 *             content within a few bins of fs / 2D aliases (same section).
 *   lgD = 0   is the sample-crop call, bit for bit.
 *   LIMITS    nB = ulcx_crop_blocks(BS', nSamples) must be at most maxBlocksPerCall - 1.
 *   d_bits    [n][nB]: the sizes of the FULL blocks, entry for entry what a sample-crop row over the same blocks reports.
 *   UNTRUSTED ROWS, STATE, ORDER, ALLOCATION: the sample-crop calls' - untrusted rows and tables give rows of zeros and touch
 *             nothing else; no stream's state is read or changed, the call mixes freely with streaming decodes on the object; it is
 *             asynchronous on hipStream (the rows, the walk, the synthesis); nothing is allocated after the first call at a ratio
 *             (that call builds the tables of BS' and the lapping scratch of its synthesis kernel).
 *   REFUSALS  ULCX_ERR_ARG before any device work: lgD outside 0 .. 3, ulcx_lowrate_block(BlockSize, lgD) == 0, and every refusal of
 *             the sample-crop call.  The host forms also refuse a start beyond the file's indexBlocks * BS'.
 *   ALIGNMENT the sample-crop calls'. */
#ifndef ULC_AMD_LOWRATE_H
#define ULC_AMD_LOWRATE_H
#include "ulc_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

int  ulcx_lowrate_block(int BlockSize, int lgD);   /* BlockSize >> lgD for 0 <= lgD <= 3 when that is a legal BlockSize (256 or more), else 0; host arithmetic */
int  ulcx_decode_crops_lowrate_dev(ulcx_decoder *dec, int nFiles,
                                   const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                                   const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                                   int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                   int nSamples, int lgD, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_lowrate_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                         const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                         const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                         int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                         int nSamples, int lgD, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_lowrate_host(ulcx_decoder *dec, int nFiles,
                                    const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                    const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                    int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                    int nSamples, int lgD, float *h_pcm, int32_t *h_bits);   /* synchronous */
int  ulcx_decode_crops_lowrate_ragged_dev(ulcx_decoder *dec, int nFiles,
                                          const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                          const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                          const int32_t *d_indexBlocks /* [nFiles] */,
                                          int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                          int nSamples, int lgD, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_lowrate_ragged_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                                const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                                const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs,
                                                const int32_t *d_indexBlocks,
                                                int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                                int nSamples, int lgD, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_lowrate_ragged_host(ulcx_decoder *dec, int nFiles,
                                           const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                           const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                           const int32_t *h_indexBlocks,
                                           int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                           int nSamples, int lgD, float *h_pcm, int32_t *h_bits);   /* synchronous */

#ifdef __cplusplus
}
#endif
#endif
