// ulcx_units.hip - TEST-ONLY device module (libulcx_units.so; tests/test_gpu_units.py).  Never linked into libulc_amd.so
// or ulcx-tool.  Thin kernels that apply the product's own small device functions - included from the product's headers,
// no copies - element-wise to a device array or to a generated range of bit patterns lo, lo + stride, ..., and store
// the results.  Built with the product's flags, so the functions are compiled as the codec's kernels compile them.
//
// Every entry point returns 0 or a hipError_t: the launch error, else that of the synchronise behind it.  No kernel
// forms an address from its data: indices come from the thread id, bounded by the element count the caller passes
// (the caller sizes the buffers from the same count); the one data-dependent look-up, rng_jump's, stays inside the
// table by construction (digit position < 8, digit < 16, byte < 256).
#include "ulcx_enc_dev.h"
#include "ulcx_dec_dev.h"
#include "ulcx_rng_tables.h"

#define UT 256

// functions of one 32-bit pattern (ulcx_units_f32)
enum { UF_EXPF, UF_EXPF_T, UF_LOGF, UF_FASTLOG, UF_QUANT_U, UF_QUANT_COEF_U, UF_QUANT_COEF, UF_BUILD_QUANTIZER, UF_TO_PCM16, UF_KEY_ORD,
       UF_EXPAND_QUANTIZER, UF_COUNT };

template <int FN> __device__ __forceinline__ uint32_t unit_apply(uint32_t u, int arg, const unsigned long long *sexp) {
    const float x = __uint_as_float(u);
    switch (FN) {
    case UF_EXPF:             return __float_as_uint(ulcx_expf(x));
    case UF_EXPF_T:           return __float_as_uint(ulcx_expf_t(x, sexp));
    case UF_LOGF:             return __float_as_uint(ulcx_logf(x));
    case UF_FASTLOG:          return __float_as_uint(fastlog(x));
    case UF_QUANT_U:          return (uint32_t)quant_u(x);
    case UF_QUANT_COEF_U:     return (uint32_t)quant_coef_u(x, arg);
    case UF_QUANT_COEF:       return (uint32_t)quant_coef(x, arg);
    case UF_BUILD_QUANTIZER:  return (uint32_t)build_quantizer(x);
    case UF_TO_PCM16:         return (uint32_t)(int)to_pcm16(x);
    case UF_KEY_ORD:          return key_ord(x);
    case UF_EXPAND_QUANTIZER: return __float_as_uint(expand_quantizer((int)u));
    }
    return 0;
}

// in != NULL: out[i] = f(in[i]); else out[i] = f((uint32_t)(lo + i * stride)), i < n
template <int FN> __global__ __launch_bounds__(UT) void k_unit_f32(const uint32_t *in, unsigned long long lo, unsigned long long stride, long long n, int arg, uint32_t *out) {
    __shared__ unsigned long long sexp[32];                // expf's 2^(i/32) table staged as k_nsums stages it
    if (FN == UF_EXPF_T) {
        if (threadIdx.x < 32) sexp[threadIdx.x] = ulcx_exp2f_tab[threadIdx.x];
        __syncthreads();
    }
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    const uint32_t u = in ? in[i] : (uint32_t)(lo + (unsigned long long)i * stride);
    out[i] = unit_apply<FN>(u, arg, sexp);
}

__global__ __launch_bounds__(UT) void k_unit_log(const uint64_t *in, long long n, uint64_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    out[i] = ulcx_d2u(ulcx_log(ulcx_u2d(in[i])));
}

// every field of decode_code for the windows lo .. lo + n - 1: out[i][12] in the order of UNIT_CODE_FIELDS (tests)
__global__ __launch_bounds__(UT) void k_unit_decode_code(uint32_t lo, long long n, int first, int32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    const Code k = decode_code(lo + (uint32_t)i, first != 0);
    int32_t *o = out + i * 12;
    o[0] = k.len; o[1] = k.n; o[2] = k.np; o[3] = k.l; o[4] = k.dn; o[5] = k.sv; o[6] = k.qnew;
    o[7] = k.plain; o[8] = k.zrun; o[9] = k.n8; o[10] = k.tail; o[11] = k.stop;
}

// plain_prefix of the windows (lo + i) | top << 28 (top = the eighth nybble, which is no part of the window)
__global__ __launch_bounds__(UT) void k_unit_plain_prefix(uint32_t lo, uint32_t top, long long n, uint8_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    out[i] = (uint8_t)plain_prefix((lo + (uint32_t)i) | (top << 28));
}

// sel[ire][im] = sel_key(re, m, ch), ref[ire][im] = key_ord(final_key(key0_of(re), m, ch)); with mdiag the masking level of
// column 0 is -2 * fastlog(re^2) of the row's own coefficient (the level at which the two terms of the key cancel)
__global__ __launch_bounds__(UT) void k_unit_sel_key(const uint32_t *re, long long nre, const uint32_t *m, int nm, int mdiag, int ch, uint32_t *sel, uint32_t *ref) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= nre * nm) return;
    const int im = (int)(i % nm);
    const float r = __uint_as_float(re[i / nm]);
    const float lvl = (mdiag && im == 0) ? -2.0f * fastlog(r * r) : __uint_as_float(m[im]);
    sel[i] = sel_key(r, lvl, ch);
    ref[i] = key_ord(final_key(key0_of(r), lvl, ch));
}

// out[is][in] = rng_jump(s[is], len[in])
__global__ __launch_bounds__(UT) void k_unit_rng_jump(const uint32_t *jt, const uint32_t *s, long long ns, const uint32_t *len, long long nl, uint32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= ns * nl) return;
    out[i] = rng_jump(jt, s[i / nl], len[i % nl]);
}
// out[i] = rng_jump(s[i], len[i])
__global__ __launch_bounds__(UT) void k_unit_rng_jump_each(const uint32_t *jt, const uint32_t *s, const uint32_t *len, long long n, uint32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    out[i] = rng_jump(jt, s[i], len[i]);
}

// The wave primitives, one value per lane, workgroups of four waves; n is a multiple of 256 (every wave is full: the row
// shifts read all 64 lanes).  out[7][n]: wave_sum_i32, wave_min_u32, wave_max_u32, wave_scan_add, wave_scan_max,
// wave_excl_scan and its total.
__global__ __launch_bounds__(UT) void k_unit_wave(const uint32_t *in, long long n, uint32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    const uint32_t v = in[i];
    out[i] = (uint32_t)wave_sum_i32((int)v);
    out[n + i] = wave_min_u32(v);
    out[2 * n + i] = wave_max_u32(v);
    out[3 * n + i] = wave_scan_add(v);
    out[4 * n + i] = wave_scan_max(v);
    int total;
    out[5 * n + i] = (uint32_t)wave_excl_scan((int)v, threadIdx.x & 63, total);
    out[6 * n + i] = (uint32_t)total;
}

__global__ __launch_bounds__(UT) void k_unit_noise_q(const float *sum, const float *sumw, const float *q, long long n, int32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    out[i] = noise_q_from_sums(sum[i], sumw[i], q[i]);
}
// sums[i][5] = {sx, sx2, sxy, sy, sw}; out[i][2] = {noiseQ, noiseDecay}, both 0 in front of the call as in the writer
__global__ __launch_bounds__(UT) void k_unit_hfext(const float *sums, const float *q, long long n, int32_t *out) {
    const long long i = (long long)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    const float *s = sums + i * 5;
    int nq = 0, nd = 0;
    hfext_from_sums(s[0], s[1], s[2], s[3], s[4], q[i], nq, nd);
    out[2 * i] = nq; out[2 * i + 1] = nd;
}

// The view of a corpus (corpus_file, file_block) for the files f < s.nFiles of caller-given tables: out[f][4 + 2 * nk] =
// {base - s.pay, row - s.index in entries, avail, nI, then {off, ext} of block ks[j], j < nk}.  No payload byte is read (s.pay
// is only ever an address to count from).  A view whose row leaves the index is not followed: the lookups store -1 (the test's
// model never has it), so a wrong view fails the test instead of reading outside the caller's buffers.
__global__ __launch_bounds__(UT) void k_unit_corpus(UlcxCorpus s, const int32_t *ks, int nk, long long *out) {
    const int f = blockIdx.x * UT + threadIdx.x;
    if (f >= s.nFiles) return;
    const CorpusFile cf = corpus_file(s, (size_t)f, s.payOffs != nullptr);
    long long *o = out + (size_t)f * (4 + 2 * nk);
    const long long rowAt = cf.row - s.index;
    o[0] = cf.base - s.pay; o[1] = rowAt; o[2] = cf.avail; o[3] = cf.nI;
    const bool rowInside = cf.nI >= 0 && rowAt >= 0 && rowAt + cf.nI + (cf.ok ? 1 : 0) <= s.idxTotal;
    for (int j = 0; j < nk; j++) {
        const FileBlock b = rowInside ? file_block(cf, ks[j]) : FileBlock{ -1, -1 };
        o[4 + 2 * j] = b.off; o[5 + 2 * j] = b.ext;
    }
}

static int unit_done() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}
static unsigned unit_grid(long long n) { return (unsigned)((n + UT - 1) / UT); }
#define UNIT_NMAX (1ll << 31)                              // elements per launch (the callers chunk far below it)

static uint32_t *g_jumpT = nullptr;                        // the library's own tables (build_rng_tables), built once
static int unit_jump_tables() {
    if (g_jumpT) return 0;
    std::vector<uint32_t> jt;
    build_rng_tables(jt);
    hipError_t e = hipMalloc((void **)&g_jumpT, jt.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(g_jumpT, jt.data(), jt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (g_jumpT) (void)hipFree(g_jumpT); g_jumpT = nullptr; }
    return (int)e;
}

extern "C" {
int ulcx_units_function_count(void) { return UF_COUNT; }

// fn: UF_*; arg: the limit of quant_coef_u / quant_coef.  in == NULL: the patterns lo + i * stride (mod 2^32), i < n.
int ulcx_units_f32(int fn, int arg, const uint32_t *in, unsigned long long lo, unsigned long long stride, long long n, uint32_t *out) {
    if (n < 0 || n > UNIT_NMAX || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
#define UNIT_CASE(F) case F: k_unit_f32<F><<<unit_grid(n), UT>>>(in, lo, stride, n, arg, out); break;
    switch (fn) {
    UNIT_CASE(UF_EXPF) UNIT_CASE(UF_EXPF_T) UNIT_CASE(UF_LOGF) UNIT_CASE(UF_FASTLOG) UNIT_CASE(UF_QUANT_U) UNIT_CASE(UF_QUANT_COEF_U)
    UNIT_CASE(UF_QUANT_COEF) UNIT_CASE(UF_BUILD_QUANTIZER) UNIT_CASE(UF_TO_PCM16) UNIT_CASE(UF_KEY_ORD) UNIT_CASE(UF_EXPAND_QUANTIZER)
    default: return (int)hipErrorInvalidValue;
    }
#undef UNIT_CASE
    return unit_done();
}
int ulcx_units_log(const uint64_t *in, long long n, uint64_t *out) {
    if (n < 0 || n > UNIT_NMAX || !in || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_log<<<unit_grid(n), UT>>>(in, n, out);
    return unit_done();
}
int ulcx_units_decode_code(uint32_t lo, long long n, int first, int32_t *out) {
    if (n < 0 || n > (1ll << 26) || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_decode_code<<<unit_grid(n), UT>>>(lo, n, first, out);
    return unit_done();
}
int ulcx_units_plain_prefix(uint32_t lo, uint32_t top, long long n, uint8_t *out) {
    if (n < 0 || n > (1ll << 28) || top > 15u || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_plain_prefix<<<unit_grid(n), UT>>>(lo, top, n, out);
    return unit_done();
}
int ulcx_units_sel_key(const uint32_t *re, long long nre, const uint32_t *m, int nm, int mdiag, int ch, uint32_t *sel, uint32_t *ref) {
    if (nre < 0 || nm < 1 || nre * nm > UNIT_NMAX || !re || !m || !sel || !ref) return (int)hipErrorInvalidValue;
    if (nre == 0) return 0;
    k_unit_sel_key<<<unit_grid(nre * nm), UT>>>(re, nre, m, nm, mdiag, ch, sel, ref);
    return unit_done();
}
int ulcx_units_rng_jump(const uint32_t *s, long long ns, const uint32_t *len, long long nl, uint32_t *out) {
    if (ns < 0 || nl < 0 || ns > UNIT_NMAX || nl > UNIT_NMAX || ns * nl > UNIT_NMAX || !s || !len || !out) return (int)hipErrorInvalidValue;
    if (ns * nl == 0) return 0;
    if (int e = unit_jump_tables()) return e;
    k_unit_rng_jump<<<unit_grid(ns * nl), UT>>>(g_jumpT, s, ns, len, nl, out);
    return unit_done();
}
int ulcx_units_rng_jump_each(const uint32_t *s, const uint32_t *len, long long n, uint32_t *out) {
    if (n < 0 || n > UNIT_NMAX || !s || !len || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (int e = unit_jump_tables()) return e;
    k_unit_rng_jump_each<<<unit_grid(n), UT>>>(g_jumpT, s, len, n, out);
    return unit_done();
}
int ulcx_units_wave(const uint32_t *in, long long n, uint32_t *out) {
    if (n < 0 || n > UNIT_NMAX / 8 || (n % UT) != 0 || !in || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_wave<<<(unsigned)(n / UT), UT>>>(in, n, out);
    return unit_done();
}
int ulcx_units_noise_q(const float *sum, const float *sumw, const float *q, long long n, int32_t *out) {
    if (n < 0 || n > UNIT_NMAX || !sum || !sumw || !q || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_noise_q<<<unit_grid(n), UT>>>(sum, sumw, q, n, out);
    return unit_done();
}
// payOffs != NULL: a ragged corpus (payBytes, payStride and indexStride are not looked at), else a strided one (payTotal is not); every table on the
// device, index of idxTotal entries (strided: nFiles * indexStride); out[nFiles][4 + 2 * nk]
int ulcx_units_corpus(int nFiles, long long payTotal, long long payStride, const int32_t *payBytes, const int64_t *payOffs, const ulcx_index_entry *index,
                      long long idxTotal, int indexStride, const int64_t *idxOffs, const int32_t *indexBlocks, const int32_t *ks, int nk, long long *out) {
    if (nFiles < 1 || nFiles > (1 << 20) || nk < 0 || nk > 64 || !index || !indexBlocks || !ks || !out || idxTotal < 0) return (int)hipErrorInvalidValue;
    if (payOffs ? !idxOffs : (!payBytes || indexStride < 1 || idxTotal != (long long)nFiles * indexStride)) return (int)hipErrorInvalidValue;
    UlcxCorpus s = payOffs ? ulcx_corpus_ragged(nFiles, (const uint8_t *)index, payTotal, payOffs, index, idxTotal, idxOffs, indexBlocks)
                           : ulcx_corpus_strided(nFiles, (const uint8_t *)index, payStride, payBytes, index, indexStride, indexBlocks);
    k_unit_corpus<<<unit_grid(nFiles), UT>>>(s, ks, nk, out);
    return unit_done();
}
int ulcx_units_hfext(const float *sums, const float *q, long long n, int32_t *out) {
    if (n < 0 || n > UNIT_NMAX / 8 || !sums || !q || !out) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    k_unit_hfext<<<unit_grid(n), UT>>>(sums, q, n, out);
    return unit_done();
}
}
