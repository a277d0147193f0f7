/* Host-side referee of tests/test_gpu_units.py: the oracle's scalar helpers (liboracle.so, pinned to the reference by
 * tests/test_oracle_pinned.py) applied over whole arrays and compared with results computed elsewhere (on the device).
 * A Python loop over ctypes scalars would take minutes for the 70 M points of a sweep.  Built with -ffp-contract=off.
 *
 * Where the C reference is undefined the comparison is left out and counted (`skipped`):
 *   quant_u, quant_coef_u, quant_coef   (int) of 0.5f + sqrtf(|v| - 0.25f) when that is 2^31 or more, +-inf included
 *                                       (NaN is inside the domain: `v >= 0.5f` is false, the result is 0)
 *   build_quantizer                     maxv must be positive and finite (logf of 0 / negative / inf / NaN -> (int) of
 *                                       a non-finite value)
 *   to_pcm16                            the argument must be finite (lrintf of NaN is unspecified)
 * The callers compute how many patterns of their sweep lie outside each domain and assert that no more were skipped. */
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../oracle/ulc_oracle.h"

enum { UF_FASTLOG = 3, UF_QUANT_U = 4, UF_QUANT_COEF_U = 5, UF_QUANT_COEF = 6, UF_BUILD_QUANTIZER = 7, UF_TO_PCM16 = 8 };   /* as ulcx_units.hip */

static float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int quant_defined(float v) { return !(v >= 0.5f) || (0.5f + sqrtf(v - 0.25f) < 0x1.0p31f); }

/* the WAV writer's conversion (tools/WavIO_Helper.c:56-63): lrintf(clamp(x * 2^15, -32768, 32767)) */
static int32_t wav_pcm16(float x) {
    float v = x * 0x1.0p+15f;
    v = (v < -32768.0f) ? -32768.0f : (v > 32767.0f) ? 32767.0f : v;
    return (int32_t)(int16_t)lrintf(v);
}

/* got[i] = the device's result for the pattern in[i] (in == NULL: lo + i * stride mod 2^32).  Returns the number of
 * mismatches inside the function's domain; first bad argument / the oracle's value for it in *bad / *want. */
long long ref_cmp_f32(int fn, int arg, const uint32_t *got, const uint32_t *in, uint64_t lo, uint64_t stride, long long n,
                      uint32_t *bad, uint32_t *want, long long *skipped) {
    long long m = 0, sk = 0;
    for (long long i = 0; i < n; i++) {
        const uint32_t u = in ? in[i] : (uint32_t)(lo + (uint64_t)i * stride);
        const float x = u2f(u);
        uint32_t r;
        switch (fn) {
        case UF_FASTLOG:         r = f2u(orc_fastlog(x)); break;
        case UF_QUANT_U:         if (!quant_defined(x)) { sk++; continue; } r = (uint32_t)orc_companded_quantize_unsigned(x); break;
        case UF_QUANT_COEF_U:    if (!quant_defined(x)) { sk++; continue; } r = (uint32_t)orc_quant_coef_unsigned(x, arg); break;
        case UF_QUANT_COEF:      if (!quant_defined(fabsf(x))) { sk++; continue; } r = (uint32_t)orc_quant_coef(x, arg); break;
        case UF_BUILD_QUANTIZER: if (!(x > 0.0f && x < INFINITY)) { sk++; continue; } r = (uint32_t)orc_build_quantizer(x); break;
        case UF_TO_PCM16:        if (!isfinite(x)) { sk++; continue; } r = (uint32_t)wav_pcm16(x); break;
        default: return -1;
        }
        if (got[i] != r) { if (!m) { if (bad) *bad = u; if (want) *want = r; } m++; }
    }
    if (skipped) *skipped = sk;
    return m;
}

/* got[is][k] (k < nlen) against orc_xorshift32 applied k times to s[is]; first bad {state index, length} in bad[2] */
long long ref_cmp_rng_iter(const uint32_t *got, const uint32_t *s, long long ns, long long nlen, long long *bad, uint32_t *want) {
    long long m = 0;
    for (long long is = 0; is < ns; is++) {
        uint32_t st = s[is];
        for (long long k = 0; k < nlen; k++) {
            if (got[is * nlen + k] != st) { if (!m) { if (bad) { bad[0] = is; bad[1] = k; } if (want) *want = st; } m++; }
            st = orc_xorshift32(st);
        }
    }
    return m;
}

/* Noise-fill cases: case i takes cnt[i] {w, w*logNoise} pairs from pairs + 2 * off[i].  Forms the sums the kernels hand
 * to noise_q_from_sums / hfext_from_sums - binary32, sequential, in the kernels' order (ulcx_enc_wr.hip get_noise_q /
 * get_hfext) - into sum2[i] = {sum, sumw} and sum5[i] = {sx, sx2, sxy, sy, sw}, and gives the same pairs to the pinned
 * orc_get_noise_q / orc_get_hfext_params: refq[i], refhf[i] = {NoiseQ, NoiseDecay} (zero in front of the call, as the
 * writer has them). */
void ref_noise_cases(const float *pairs, const int32_t *off, const int32_t *cnt, const float *q, long long n,
                     float *sum2, float *sum5, int32_t *refq, int32_t *refhf) {
    for (long long i = 0; i < n; i++) {
        const float *p = pairs + 2 * (size_t)off[i];
        float sum = 0.0f, sumw = 0.0f, sx = 0.0f, sx2 = 0.0f, sxy = 0.0f, sy = 0.0f, sw = 0.0f;
        for (int k = 0; k < cnt[i]; k++) {
            const float w = p[2 * k], wy = p[2 * k + 1], x = k * 2.0f;
            sum += wy; sumw += w;
            const float wx = w * x;
            sx += wx; sx2 += wx * x; sxy += x * wy; sy += wy; sw += w;
        }
        sum2[2 * i] = sum; sum2[2 * i + 1] = sumw;
        sum5[5 * i] = sx; sum5[5 * i + 1] = sx2; sum5[5 * i + 2] = sxy; sum5[5 * i + 3] = sy; sum5[5 * i + 4] = sw;
        refq[i] = orc_get_noise_q(p, 0, 2 * cnt[i], q[i]);
        int nq = 0, nd = 0;
        orc_get_hfext_params(p, 0, 2 * cnt[i], q[i], &nq, &nd);
        refhf[2 * i] = nq; refhf[2 * i + 1] = nd;
    }
}

/* obvious loop: leading nybbles (low first, at most 7) of w that are none of 0h 1h 8h Fh */
static int plain_prefix_ref(uint32_t w) {
    int k = 0;
    while (k < 7) {
        const unsigned v = (w >> (4 * k)) & 15u;
        if (v == 0x0 || v == 0x1 || v == 0x8 || v == 0xF) break;
        k++;
    }
    return k;
}
/* got[i] for the window (lo + i) | top << 28; first bad window in *bad */
long long ref_cmp_plain_prefix(const uint8_t *got, uint32_t lo, uint32_t top, long long n, uint32_t *bad, int *want) {
    long long m = 0;
    for (long long i = 0; i < n; i++) {
        const uint32_t w = (lo + (uint32_t)i) | (top << 28);
        const int r = plain_prefix_ref(w);
        if (got[i] != r) { if (!m) { if (bad) *bad = w; if (want) *want = r; } m++; }
    }
    return m;
}
