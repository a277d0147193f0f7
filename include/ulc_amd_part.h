/* ulc_amd_part.h — mid and side crops: one coded channel of every channel pair, straight from the synthesis, no un-mix.
 *
 * The codec codes channels in pairs, a = (L + R) / 2 and b = (L - R) / 2, and the reference decoder holds a and b in DstData up to
 * its last loop, which forms a + b and a - b (ulcDecoder.c:279-289).  The mid channel IS the mono downmix, and it lies in the file
 * as a coded channel of its own: one dequantisation, one inverse transform and one plane of stores per pair.  These entries are
 * the low-rate sample-crop calls of ulc_amd_lowrate.h (ulcx_decode_crops_lowrate_*) with one further argument, int part, behind lgD.
 *
 *   OUTPUT    d_pcm [n][nOut][nSamples], nOut = ulcx_part_channels(nChan, part).  Output plane j is coded channel 2 j + part; for an
 *             odd nChan and ULCX_PART_MID the last, unpaired channel is the last plane.
 *   ROWS, d_len, d_bits, the zeros behind the length / the file's end / a corrupt block, UNTRUSTED ROWS and tables, STATE, ORDER,
 *             ALLOCATION, ALIGNMENT, LIMITS: the low-rate calls', word for word; lgD is theirs too - rows and nSamples count samples of
 *             the reduced stream, lgD = 0 is full rate.
 *   A LIVE SAMPLE is, bit for bit, what the reference decoder holds in DstData[Chan * BlockSize + n] for Chan = 2 j + part in front of
 *             its un-mix loop; at lgD > 0 the decoder of BlockSize BS >> lgD whose TransformBuffer holds the low bins
 *             (ulc_amd_lowrate.h).  Equivalently: ulcx_decode_crops_spectra_dev WITHOUT ULCX_SPECTRA_LR, the plane of channel
 *             2 j + part and of every sub-block its low bins, then ulcx_synth_spectra_dev with ULCX_SYNTH_WARM on a ONE-channel
 *             decoder of BlockSize BS >> lgD.  The noise is the full decode's: the generator has drawn for every channel and every
 *             coefficient in front of the unit.
 *   MID       is (L + R) / 2 of the decoded stereo only up to the two float32 roundings of the un-mix (L = fl(a + b), R = fl(a - b),
 *             then their sum): |(L + R) / 2 - a| <= 2^-24 max(|a|, |b|) for the fold formed WITHOUT rounding; a fold in float32 rounds a third
 *             time, fl(L + R), and may lie a further half ulp of L + R away.  Not bit for bit.  A mono corpus under ULCX_PART_MID is the low-rate / sample-crop call itself, bit for bit.
 *   PCM16     converts the plane as the other calls convert a channel.
 *   TIME      the low-rate calls' ("Low-rate crops" and "Mid and side crops").
 *   LAUNCH    the crop walk as it is, then ONE WORKGROUP PER ROW WITHOUT A CUT: for stereo with BlockSize >> lgD up to 4096 a workgroup
 *             of one wave (k_dpart: one FFT array, no barrier between waves), else the general kernel (k_dgen) over the part's
 *             channels.  Many rows fill the device; a few long rows do not - there the stereo call, which cuts its rows, is faster
 *             (64 rows x 31 blocks: 0.83 against 0.45 ms; 4096 rows: 1.66 against 1.97 ms - profiles/part_bench.txt).  ulcx_decoder_last_cut reports 0, 0 behind a part call.
 *   REFUSALS  ULCX_ERR_ARG before any device work: part outside 0 .. 1, ulcx_part_channels(nChan, part) == 0 (the side of a mono
 *             corpus), and every refusal of the low-rate call. */
#ifndef ULC_AMD_PART_H
#define ULC_AMD_PART_H
#include "ulc_amd_lowrate.h"
#ifdef __cplusplus
extern "C" {
#endif

#define ULCX_PART_MID  0
#define ULCX_PART_SIDE 1

int  ulcx_part_channels(int nChan, int part);   /* planes of the output: (nChan + 1 - part) / 2 for part 0 / 1 and nChan 1 .. 255, else 0; host arithmetic */
int  ulcx_decode_crops_part_dev(ulcx_decoder *dec, int nFiles,
                                const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes /* [nFiles] */,
                                const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks /* [nFiles] */,
                                int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                int nSamples, int lgD, int part, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_part_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                      const uint8_t *d_payload, long long payloadStride, const int32_t *d_payloadBytes,
                                      const ulcx_index_entry *d_index, int indexStride, const int32_t *d_indexBlocks,
                                      int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                      int nSamples, int lgD, int part, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_part_host(ulcx_decoder *dec, int nFiles,
                                 const uint8_t *h_payload, long long payloadStride, const int32_t *h_payloadBytes,
                                 const ulcx_index_entry *h_index, int indexStride, const int32_t *h_indexBlocks,
                                 int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                 int nSamples, int lgD, int part, float *h_pcm, int32_t *h_bits);   /* synchronous */
int  ulcx_decode_crops_part_ragged_dev(ulcx_decoder *dec, int nFiles,
                                       const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs /* [nFiles+1] */,
                                       const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs /* [nFiles+1] */,
                                       const int32_t *d_indexBlocks /* [nFiles] */,
                                       int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len /* optional */,
                                       int nSamples, int lgD, int part, float *d_pcm, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_part_ragged_dev_pcm16(ulcx_decoder *dec, int nFiles,
                                             const uint8_t *d_payload, long long payloadTotal, const int64_t *d_payloadOffs,
                                             const ulcx_index_entry *d_index, long long indexTotal, const int64_t *d_indexOffs,
                                             const int32_t *d_indexBlocks,
                                             int n, const int32_t *d_file, const int64_t *d_start, const int32_t *d_len,
                                             int nSamples, int lgD, int part, int16_t *d_pcm16, int32_t *d_bits, void *hipStream);
int  ulcx_decode_crops_part_ragged_host(ulcx_decoder *dec, int nFiles,
                                        const uint8_t *h_payload, long long payloadTotal, const int64_t *h_payloadOffs,
                                        const ulcx_index_entry *h_index, long long indexTotal, const int64_t *h_indexOffs,
                                        const int32_t *h_indexBlocks,
                                        int n, const int32_t *h_file, const int64_t *h_start, const int32_t *h_len,
                                        int nSamples, int lgD, int part, float *h_pcm, int32_t *h_bits);   /* synchronous */

#ifdef __cplusplus
}
#endif
#endif
