/* Definitions behind standin/Fourier.h: the two transforms the reference's libulc calls, forwarded to the project's
 * fourier spec v2 (orc_fourier.c).  Test infrastructure only. */
#include "standin/Fourier.h"
#include "ulc_oracle.h"

void Fourier_MDCT_MDST(float *MDCT, float *MDST, const float *New, float *Lap, float *Tmp, int N, int Overlap) { orc_mdct_mdst(MDCT, MDST, New, Lap, Tmp, N, Overlap); }
void Fourier_IMDCT(float *Out, const float *In, float *Lap, float *Tmp, int N, int Overlap) { orc_imdct(Out, In, Lap, Tmp, N, Overlap); }
