/*
 * Fourier.h — written by this project, TEST INFRASTRUCTURE ONLY (see oracle/README.md).
 *
 * Stands in for the header of the absent libfourier submodule so that the reference's
 * libulc sources that include it (ulcEncoder.c, ulcEncoder_BlockTransform.c,
 * ulcEncoder_Encode.c, ulcDecoder.c) compile in place.  They call exactly two functions
 * from it; these are their prototypes, as the call sites use them.  The definitions
 * (ref_fourier_standin.c) forward to this project's "fourier spec v2" (orc_fourier.c,
 * DESIGN.md §3), not to libfourier, whose operation order is unknown: a build over this
 * header pins everything but the transforms.
 */
#pragma once

void Fourier_MDCT_MDST(float *MDCT, float *MDST, const float *New, float *Lap, float *Tmp, int N, int Overlap);
void Fourier_IMDCT(float *Out, const float *In, float *Lap, float *Tmp, int N, int Overlap);
