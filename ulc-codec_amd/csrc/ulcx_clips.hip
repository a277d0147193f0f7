// ulcx_clips.hip — the write side of a resident corpus (include/ulc_amd.h, "Clips" and "Strided corpus -> ragged corpus").
//
// ulcx_encode_clips_*: rows are whole clips in samples, channels-first, each at its own length.  The encoder's kernels are
// not touched: they still read [rows][K][BlockSize][nChan] interleaved blocks, here from a staging buffer of the object, and
// write per-block slots, here into slots of the object.  Three kernels of this file stand around them:
//   k_clip_begin     the shadow state of the call's rows to the state right after create; byte counts and largest blocks of
//                    the call's files (rows x rungs) to 0
//   k_clip_stage     planar samples of rows x blocks [k0, k0 + K) -> the interleaved chunk, zeros outside [0, L_i)
//   k_clip_append    one workgroup per file (row i under rung r is file r * n + i; the plain call: one rung): the chunk's blocks
//                    that belong to the row (behind nb_i: silence nobody asked for; behind the capacity rule: blocks that do
//                    not fit) keep their size, every other size becomes 0; the kept slots' bytes go behind the file's running
//                    payload
// The index of the chunk is then ulcx_index_slots_dev's two kernels on the masked sizes (ulcx_dec.hip).
// ulcx_analyse_clips_* / ulcx_encode_clips_spectra_* add k_clip_spec behind the launch sequence: the chunk's MDCT coefficients,
// window codes and complexities into the caller's channels-first planes.
// ulcx_encode_clips_ladder_* with a ULCX_RUNG_AUTO rung run an analysis pass in front: k_clip_cplx_sum behind each of its chunks
// (a row's complexities into one binary64 sum, in block order), k_clip_auto behind the last one (the rows' averages and the
// AUTO rungs' tables {RateKbps, avg_i}).
//
// ulcx_corpus_ragged_*: k_corpus_offsets (one workgroup: the two exclusive int64 prefix sums, the first file that does not
// fit, the totals) and k_corpus_copy (a file per workgroup).
// Plain C++ vector accesses only.
#include "ulcx_internal.h"

#define CLIP_WG 256
#define CLIP_GRID 16384

// a sample of the call's input as the encoder takes it: binary32 as it is, PCM16 as ulcx_encode_dev_pcm16 converts it on load
// (tools/WavIO_Helper.c:49-55: (float)x * 2^-15, exact)
__device__ static inline float clip_sample(float x) { return x; }
__device__ static inline float clip_sample(int16_t x) { return (float)x * 0x1.0p-15f; }
// two consecutive samples of one plane; one load where the address allows it (a plane starts at any sample)
__device__ static inline float2 clip_pair(const float *p) {
    if (((uintptr_t)p & 7u) == 0) return *(const float2 *)p;
    return make_float2(p[0], p[1]);
}
__device__ static inline float2 clip_pair(const int16_t *p) {
    if (((uintptr_t)p & 3u) == 0) { const short2 v = *(const short2 *)p; return make_float2(clip_sample((int16_t)v.x), clip_sample((int16_t)v.y)); }
    return make_float2(clip_sample(p[0]), clip_sample(p[1]));
}
__device__ static inline int clip_len(const int32_t *len, int i, int nSamples) {
    if (!len) return nSamples;
    const int l = len[i];
    return l < 0 ? 0 : l > nSamples ? nSamples : l;
}
// ulcx_clip_blocks on the device (BS a valid block size)
__device__ static inline int clip_blocks(int BS, int L) { return L >= 1 ? (int)(((long long)L + BS - 1) / BS) + 2 : 0; }

// n rows of state; nOut >= n counters (the call's files: rows x rungs); sum: the rows' complexity sums of an analysis pass, or NULL
__global__ __launch_bounds__(CLIP_WG) void k_clip_begin(float *hist, UlcxWcState *wcs, int n, int histVec, int nOut, int32_t *payBytes, int32_t *maxBlock, double *sum) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        float4 *h = (float4 *)hist + (size_t)i * histVec;
        for (int v = threadIdx.x; v < histVec; v += CLIP_WG) h[v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t *w = (uint32_t *)(wcs + i);
        // (enc_reset_state, ulcx_api.cpp: all zero, WindowCtrl of the virtual block -1 and of block 0 = 0x10)
        for (int t = threadIdx.x; t < (int)(sizeof(UlcxWcState) / 4); t += CLIP_WG)
            w[t] = (t == (int)(offsetof(UlcxWcState, wcPrev) / 4) || t == (int)(offsetof(UlcxWcState, wcCur) / 4)) ? 0x10u : 0u;
        if (threadIdx.x == 0 && sum) sum[i] = 0.0;
    }
    for (int j = blockIdx.x * CLIP_WG + threadIdx.x; j < nOut; j += gridDim.x * CLIP_WG) { payBytes[j] = 0; if (maxBlock) maxBlock[j] = 0; }
}

// Stereo: a lane takes two time steps of both planes and stores one 16-byte interleaved vector {l0, r0, l1, r1}.
// perRow = K * BS / 2 vectors of a row; the grid is rows x ceil(perRow / CLIP_WG) workgroups, row-major.
template <typename IN>
__global__ __launch_bounds__(CLIP_WG) void k_clip_stage2(const IN *pcm, const int32_t *len, int nSamples, int BS, int k0, int perRow, int wgPerRow, float4 *stage) {
    const int i = blockIdx.x / wgPerRow;
    const int j = (blockIdx.x - i * wgPerRow) * CLIP_WG + threadIdx.x;
    if (j >= perRow) return;
    const int L = clip_len(len, i, nSamples);
    const long long t = (long long)k0 * BS + 2LL * j;                // the pair's first sample in the clip
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < L) {
        const IN *l = pcm + (size_t)i * 2 * (size_t)nSamples + (size_t)t, *r = l + nSamples;
        if (t + 1 < L) { const float2 a = clip_pair(l), b = clip_pair(r); v = make_float4(a.x, b.x, a.y, b.y); }
        else { v.x = clip_sample(l[0]); v.y = clip_sample(r[0]); }
    }
    stage[(size_t)i * perRow + j] = v;
}
// Any channel count: a lane takes one time step, reads it from every plane (coalesced per plane) and stores C samples.
// perRow = K * BS time steps of a row.
template <typename IN>
__global__ __launch_bounds__(CLIP_WG) void k_clip_stage(const IN *pcm, const int32_t *len, int nSamples, int C, int BS, int k0, int perRow, int wgPerRow, float *stage) {
    const int i = blockIdx.x / wgPerRow;
    const int j = (blockIdx.x - i * wgPerRow) * CLIP_WG + threadIdx.x;
    if (j >= perRow) return;
    const int L = clip_len(len, i, nSamples);
    const long long t = (long long)k0 * BS + j;
    float *dst = stage + ((size_t)i * perRow + j) * C;
    const IN *src = pcm + (size_t)i * C * (size_t)nSamples + (size_t)(t < L ? t : 0);
    for (int ch = 0; ch < C; ch++) dst[ch] = t < L ? clip_sample(src[(size_t)ch * nSamples]) : 0.0f;
}

// n bytes from src to dst, both at any address, by the whole workgroup: 4-byte stores on dst's words, each put together from
// the one or two aligned words of src that hold its bytes; the few bytes in front of dst's first word and behind its last one
// go one by one.  (The aligned words of src that are read hold at least one byte of [src, src + n).)
__device__ static inline void wg_copy_bytes(uint8_t *dst, const uint8_t *src, int n, int tid) {
    int head = (int)((4u - ((uintptr_t)dst & 3u)) & 3u);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const int words = (n - head) >> 2;
    const uint8_t *s = src + head;
    const unsigned sh = (unsigned)((uintptr_t)s & 3u) * 8u;
    const uint32_t *sw = (const uint32_t *)(s - (sh >> 3));
    uint32_t *dw = (uint32_t *)(dst + head);
    for (int w = tid; w < words; w += CLIP_WG) {
        uint32_t x = sw[w];
        if (sh) x = (x >> sh) | (sw[w + 1] << (32u - sh));
        dw[w] = x;
    }
    const int done = head + 4 * words;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

// One workgroup per file: file i = r * n + row, the row's clip under rung r (the plain call: n files).  bits [files][K] and slots
// [files][K][slot] are the object's (what the launch sequence just wrote for blocks [k0, k0 + K) of every row under every rung);
// payBytes / maxBlock / idxBlocks are the caller's running values, per file.  A file is still growing when all its blocks so far
// were kept, idxBlocks[i] == k0; it keeps the chunk's leading blocks that are the clip's (block number below nb_row), have an
// index entry left (block number + 1 <= indexStride - 1) and fit the payload's stride - whatever the row's other files keep.
__global__ __launch_bounds__(CLIP_WG) void k_clip_append(int n, int K, int k0, int BS, int nSamples, const int32_t *len, int slot, const uint8_t *slots, int32_t *bits,
                                                         uint8_t *payload, long long stride, int32_t *payBytes, int32_t *maxBlock, int indexStride, const int32_t *idxBlocks) {
    const int i = blockIdx.x, tid = threadIdx.x;
    const int nb = clip_blocks(BS, clip_len(len, i % n, nSamples));
    int32_t *rb = bits + (size_t)i * K;
    const long long lim = stride < 0x7FFFFFFFLL ? stride : 0x7FFFFFFFLL;      // (ByteOffs and d_payloadBytes are int32)
    const int off0 = payBytes[i];
    int mx = maxBlock ? maxBlock[i] : 0;
    int m = 0;
    long long off = off0;
    if (idxBlocks[i] == k0) {
        for (; m < K; m++) {
            const int g = k0 + m, b = rb[m], by = b >> 3;
            if (g >= nb || g + 1 > indexStride - 1 || b <= 0 || (b & 7) || by > slot || off + by > lim) break;
            off += by;
            mx = by > mx ? by : mx;
        }
    }
    __syncthreads();                                                     // every lane has read the sizes and the running values
    for (int k = m + tid; k < K; k += CLIP_WG) rb[k] = 0;
    uint8_t *dst = payload + (size_t)i * (size_t)stride;
    const uint8_t *src = slots + (size_t)i * K * (size_t)slot;
    int at = off0;
    for (int k = 0; k < m; k++) {
        const int by = rb[k] >> 3;                                       // (a kept block's size is not rewritten)
        wg_copy_bytes(dst + at, src + (size_t)k * slot, by, tid);
        at += by;
    }
    if (tid == 0) { payBytes[i] = (int32_t)off; if (maxBlock) maxBlock[i] = mx; }
}

// The analysis pass of a clips ladder call with ULCX_RUNG_AUTO rungs.  A lane per row: the chunk's complexities cplx [n][K] of the
// row's own blocks (block number below nb_i, whatever a capacity keeps) go to sum[i], one after the other in block order - ONE
// chain of binary64 additions per row over the whole call (cli/ulcx_tool.c:276-291 = ulcEncodeTool.c:130,164,178).
__global__ __launch_bounds__(CLIP_WG) void k_clip_cplx_sum(int n, int K, int k0, int BS, int nSamples, const int32_t *len, const float *cplx, double *sum) {
    const int i = blockIdx.x * CLIP_WG + threadIdx.x;
    if (i >= n) return;
    const int nb = clip_blocks(BS, clip_len(len, i, nSamples));
    double s = sum[i];
    for (int k = 0; k < K && k0 + k < nb; k++) s += (double)cplx[(size_t)i * K + k];
    sum[i] = s;
}
// Behind the pass's last chunk, a lane per row: avg_i = (float)(S_i / nb_i), 0 for an empty row, to avg[i] (optional) and into
// the table of every AUTO rung: {the rung's RateKbps - its scalar one or its table's entry for the row -, avg_i}; a table row with
// RateKbps < 0 stays the VBR row it is.  tables [ULCX_MAX_RUNGS][n]; a rung without AUTO has no table here.
struct ClipAutoRungs { const float2 *src[ULCX_MAX_RUNGS]; float kbps[ULCX_MAX_RUNGS]; int nRungs; uint32_t autoMask; };
__global__ __launch_bounds__(CLIP_WG) void k_clip_auto(int n, int BS, int nSamples, const int32_t *len, const double *sum, ClipAutoRungs rg, float2 *tables, float *avg) {
    const int i = blockIdx.x * CLIP_WG + threadIdx.x;
    if (i >= n) return;
    const int nb = clip_blocks(BS, clip_len(len, i, nSamples));
    const float a = nb ? (float)(sum[i] / (double)nb) : 0.0f;
    if (avg) avg[i] = a;
    for (int r = 0; r < rg.nRungs; r++) {
        if (!((rg.autoMask >> r) & 1u)) continue;
        float2 v = make_float2(rg.kbps[r], a);
        if (rg.src[r]) { const float2 t = rg.src[r][i]; v = t.x < 0.0f ? t : make_float2(t.x, a); }
        tables[(size_t)r * n + i] = v;
    }
}

// The tap of ulcx_analyse_clips_* / ulcx_encode_clips_spectra_*.  One workgroup per (row, block of the launch, channel pair):
// the pair's two BS runs of the chunk's coef [n][K][C][BS] (what the transform left for blocks [k0, k0 + K) of every row) go to
// plane position k0 + k of out [n][C][nBlocks][BS], m + s / m - s under LR (a trailing single channel as it is).  Both sides are
// touched once: 16-byte loads and stores with the non-temporal hint, a lane's accesses 16 bytes from its neighbour's.  A block
// that is not the clip's (block number at or behind nb_i, from d_len on the device) or that no chunk holds (k >= K: the planes
// behind the call's last chunk) is zeros.  The pair-0 workgroup also moves the block's wc / cplx from [n][K] to [n][nBlocks].
// The launch covers plane blocks below nBlocks only (kOut), so nothing is written outside the planes.
typedef float clip_f4 __attribute__((ext_vector_type(4)));
template <bool LR>
__global__ __launch_bounds__(CLIP_WG) void k_clip_spec(int K, int k0, int kOut, int C, int BS, int nSamples, const int32_t *len, const float *coef,
                                                       const int32_t *wcIn, const float *cplxIn, int nBlocks, float *out, int32_t *wcOut, float *cplxOut) {
    const int pairs = (C + 1) >> 1, tid = threadIdx.x;
    const unsigned b = blockIdx.x;
    const int pair = (int)(b % (unsigned)pairs), k = (int)((b / (unsigned)pairs) % (unsigned)kOut), i = (int)(b / ((unsigned)pairs * (unsigned)kOut));
    const int g = k0 + k, ch = 2 * pair, vecs = BS >> 2;
    const bool two = ch + 1 < C;
    const bool live = k < K && g < clip_blocks(BS, clip_len(len, i, nSamples));
    const clip_f4 *src = (const clip_f4 *)(coef + (((size_t)i * K + k) * C + ch) * (size_t)BS);       // (read for a live block only)
    clip_f4 *dst0 = (clip_f4 *)(out + (((size_t)i * C + ch) * nBlocks + g) * (size_t)BS), *dst1 = dst0 + (size_t)nBlocks * vecs;
    const clip_f4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int v = tid; v < vecs; v += CLIP_WG) {
        clip_f4 x = zero, y = zero;
        if (live) {
            x = __builtin_nontemporal_load(src + v);
            if (two) {
                y = __builtin_nontemporal_load(src + vecs + v);
                if (LR) { const clip_f4 m = x, s = y; x = m + s; y = m - s; }
            }
        }
        __builtin_nontemporal_store(x, dst0 + v);
        if (two) __builtin_nontemporal_store(y, dst1 + v);
    }
    if (pair == 0 && tid == 0) {
        if (wcOut) wcOut[(size_t)i * nBlocks + g] = live ? wcIn[(size_t)i * K + k] : 0;
        if (cplxOut) cplxOut[(size_t)i * nBlocks + g] = live ? cplxIn[(size_t)i * K + k] : 0.0f;
    }
}

// ---------------------------------------------------------------------------
// Strided corpus -> ragged corpus
// ---------------------------------------------------------------------------
__device__ static inline long long corpus_file_bytes(const int32_t *payBytes, long long stride, int f) {
    const long long b = payBytes[f];
    return b < 0 ? 0 : b > stride ? stride : b;
}
__device__ static inline long long corpus_file_blocks(const int32_t *idxBlocks, int indexStride, int f) {
    const long long b = idxBlocks[f];
    return b < 0 ? 0 : b > indexStride - 1 ? indexStride - 1 : b;
}
// inclusive sum over the workgroup's CLIP_WG lanes, through LDS (scr: CLIP_WG entries)
__device__ static inline long long wg_scan_incl(long long v, long long *scr, int tid) {
    scr[tid] = v;
    __syncthreads();
    for (int d = 1; d < CLIP_WG; d <<= 1) {
        const long long add = tid >= d ? scr[tid - d] : 0;
        __syncthreads();
        scr[tid] += add;
        __syncthreads();
    }
    const long long r = scr[tid];
    __syncthreads();
    return r;
}
// ONE workgroup.  Pass 1: the inclusive sums of bytes and entries, tile by tile with a carry, into offs[f + 1].  Pass 2: the
// files that fit are a leading run (the sums never decrease): its length, and the totals laid out.  Pass 3: the files behind it
// get the empty range at the end of what was laid out, and 0 blocks.
__global__ __launch_bounds__(CLIP_WG) void k_corpus_offsets(int nFiles, long long stride, const int32_t *payBytes, int indexStride, const int32_t *idxBlocks,
                                                            long long payloadCap, long long indexCap, int64_t *payOffs, int64_t *idxOffs,
                                                            int32_t *outBlocks, int64_t *need) {
    __shared__ long long scr[CLIP_WG];
    __shared__ int nFit;
    const int tid = threadIdx.x;
    long long carryB = 0, carryE = 0;
    if (tid == 0) { payOffs[0] = 0; idxOffs[0] = 0; nFit = 0; }
    for (int f0 = 0; f0 < nFiles; f0 += CLIP_WG) {
        const int f = f0 + tid;
        const bool have = f < nFiles;
        const long long b = have ? corpus_file_bytes(payBytes, stride, f) : 0;
        const long long e = have ? corpus_file_blocks(idxBlocks, indexStride, f) + 1 : 0;
        const long long sb = carryB + wg_scan_incl(b, scr, tid), se = carryE + wg_scan_incl(e, scr, tid);
        if (have) { payOffs[f + 1] = sb; idxOffs[f + 1] = se; }
        scr[tid] = sb;
        __syncthreads();
        carryB = scr[CLIP_WG - 1];
        __syncthreads();
        scr[tid] = se;
        __syncthreads();
        carryE = scr[CLIP_WG - 1];
        __syncthreads();
    }
    if (tid == 0) { need[0] = carryB; need[1] = carryE; }
    __threadfence_block();
    __syncthreads();
    for (int f = tid; f < nFiles; f += CLIP_WG) {
        const bool fits = payOffs[f + 1] <= payloadCap && idxOffs[f + 1] <= indexCap;
        const bool next = f + 1 < nFiles && payOffs[f + 2] <= payloadCap && idxOffs[f + 2] <= indexCap;
        if (fits && !next) nFit = f + 1;                                 // (one lane at the most)
    }
    __syncthreads();
    const int fit = nFit;
    const long long endB = payOffs[fit], endE = idxOffs[fit];
    __syncthreads();
    for (int f = tid; f < nFiles; f += CLIP_WG) {
        if (f >= fit) { payOffs[f + 1] = endB; idxOffs[f + 1] = endE; outBlocks[f] = 0; }
        else outBlocks[f] = (int32_t)corpus_file_blocks(idxBlocks, indexStride, f);
    }
}
// a file per workgroup: its bytes and its entries to their places (a file that did not fit has two empty ranges)
__global__ __launch_bounds__(CLIP_WG) void k_corpus_copy(int nFiles, const uint8_t *payload, long long stride, const ulcx_index_entry *index, int indexStride,
                                                         uint8_t *outPayload, const int64_t *payOffs, ulcx_index_entry *outIndex, const int64_t *idxOffs) {
    const int tid = threadIdx.x;
    for (int f = blockIdx.x; f < nFiles; f += gridDim.x) {
        const long long p0 = payOffs[f], nB = payOffs[f + 1] - p0, i0 = idxOffs[f], nE = idxOffs[f + 1] - i0;
        if (nB > 0) wg_copy_bytes(outPayload + p0, payload + (size_t)f * (size_t)stride, (int)nB, tid);
        const uint2 *src = (const uint2 *)(index + (size_t)f * indexStride);      // (an entry: two 4-byte words, 4-byte aligned)
        uint32_t *dst = (uint32_t *)(outIndex + i0);
        for (long long k = tid; k < nE; k += CLIP_WG) {
            const uint32_t *s = (const uint32_t *)(src + k);
            dst[2 * k] = s[0]; dst[2 * k + 1] = s[1];
        }
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ulcx_set_error("%s: %s", #x, hipGetErrorString(e_)); return ULCX_ERR_HIP; } } while (0)
static unsigned clip_grid(int n) { return (unsigned)(n < CLIP_GRID ? n : CLIP_GRID); }

int ulcx_clips_begin_launch(float *hist, UlcxWcState *wcs, int n, int C, int BS, int nOut, int32_t *d_payloadBytes, int32_t *d_maxBlock, double *sum, hipStream_t st) {
    hipLaunchKernelGGL(k_clip_begin, dim3(clip_grid(n)), dim3(CLIP_WG), 0, st, hist, wcs, n, 2 * BS * C / 4, nOut, d_payloadBytes, d_maxBlock, sum);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_clips_stage_launch(const float *d_pcm, const int16_t *d_pcm16, const int32_t *d_len, int nSamples, int n, int C, int BS, int k0, int K,
                            float *stage, hipStream_t st) {
    const long long perRow = (long long)K * BS / (C == 2 ? 2 : 1), wgPerRow = (perRow + CLIP_WG - 1) / CLIP_WG;
    if (perRow > 0x7FFFFFFFLL || wgPerRow * n > 0x7FFFFFFFLL) { ulcx_set_error("ulcx_encode_clips: %d rows of %d blocks are more than one chunk takes", n, K); return ULCX_ERR_ARG; }
    const dim3 grid((unsigned)(wgPerRow * n));
    if (C == 2 && d_pcm) hipLaunchKernelGGL(k_clip_stage2<float>, grid, dim3(CLIP_WG), 0, st, d_pcm, d_len, nSamples, BS, k0, (int)perRow, (int)wgPerRow, (float4 *)stage);
    else if (C == 2) hipLaunchKernelGGL(k_clip_stage2<int16_t>, grid, dim3(CLIP_WG), 0, st, d_pcm16, d_len, nSamples, BS, k0, (int)perRow, (int)wgPerRow, (float4 *)stage);
    else if (d_pcm) hipLaunchKernelGGL(k_clip_stage<float>, grid, dim3(CLIP_WG), 0, st, d_pcm, d_len, nSamples, C, BS, k0, (int)perRow, (int)wgPerRow, stage);
    else hipLaunchKernelGGL(k_clip_stage<int16_t>, grid, dim3(CLIP_WG), 0, st, d_pcm16, d_len, nSamples, C, BS, k0, (int)perRow, (int)wgPerRow, stage);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_clips_append_launch(int n, int nRungs, int K, int k0, int BS, int nSamples, const int32_t *d_len, int slot, const uint8_t *slots, int32_t *bits,
                             uint8_t *d_payload, long long stride, int32_t *d_payloadBytes, int32_t *d_maxBlock, int indexStride, const int32_t *d_indexBlocks,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_clip_append, dim3((unsigned)n * (unsigned)nRungs), dim3(CLIP_WG), 0, st, n, K, k0, BS, nSamples, d_len, slot, slots, bits, d_payload, stride,
                       d_payloadBytes, d_maxBlock, indexStride, d_indexBlocks);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_clips_cplx_sum_launch(int n, int K, int k0, int BS, int nSamples, const int32_t *d_len, const float *cplx, double *sum, hipStream_t st) {
    hipLaunchKernelGGL(k_clip_cplx_sum, dim3((unsigned)((n + CLIP_WG - 1) / CLIP_WG)), dim3(CLIP_WG), 0, st, n, K, k0, BS, nSamples, d_len, cplx, sum);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_clips_auto_launch(int n, int BS, int nSamples, const int32_t *d_len, const double *sum, const ulcx_rung *rungs, int nRungs, ulcx_rate *tables, float *d_avg,
                           hipStream_t st) {
    ClipAutoRungs rg = {};
    rg.nRungs = nRungs;
    for (int r = 0; r < nRungs; r++) {
        rg.src[r] = (const float2 *)rungs[r].rate; rg.kbps[r] = rungs[r].param0;
        if (rungs[r].reserved & ULCX_RUNG_AUTO) rg.autoMask |= 1u << r;
    }
    hipLaunchKernelGGL(k_clip_auto, dim3((unsigned)((n + CLIP_WG - 1) / CLIP_WG)), dim3(CLIP_WG), 0, st, n, BS, nSamples, d_len, sum, rg, (float2 *)tables, d_avg);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_clips_spec_launch(int n, int K, int k0, int kOut, int C, int BS, int nSamples, const int32_t *d_len, const float *coef, const int32_t *wc,
                           const float *cplx, int nBlocks, int lr, float *d_coef, int32_t *d_wc, float *d_cplx, hipStream_t st) {
    if (kOut < 1) return ULCX_OK;
    if (k0 < 0 || (long long)k0 + kOut > nBlocks) { ulcx_set_error("ulcx_clips_spec_launch: blocks %d + %d of planes %d deep", k0, kOut, nBlocks); return ULCX_ERR_ARG; }
    const long long wgs = (long long)n * kOut * ((C + 1) / 2);
    if (wgs > 0x7FFFFFFFLL) { ulcx_set_error("clip spectra: %d rows of %d blocks are more than one launch takes", n, kOut); return ULCX_ERR_ARG; }
    if (lr) hipLaunchKernelGGL(k_clip_spec<true>, dim3((unsigned)wgs), dim3(CLIP_WG), 0, st, K, k0, kOut, C, BS, nSamples, d_len, coef, wc, cplx, nBlocks, d_coef, d_wc, d_cplx);
    else hipLaunchKernelGGL(k_clip_spec<false>, dim3((unsigned)wgs), dim3(CLIP_WG), 0, st, K, k0, kOut, C, BS, nSamples, d_len, coef, wc, cplx, nBlocks, d_coef, d_wc, d_cplx);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_corpus_ragged_launch(int nFiles, const uint8_t *d_payload, long long stride, const int32_t *d_payloadBytes, const ulcx_index_entry *d_index,
                              int indexStride, const int32_t *d_indexBlocks, uint8_t *d_outPayload, long long payloadCap, int64_t *d_payloadOffs,
                              ulcx_index_entry *d_outIndex, long long indexCap, int64_t *d_indexOffs, int32_t *d_outIndexBlocks, int64_t *d_need, hipStream_t st) {
    hipLaunchKernelGGL(k_corpus_offsets, dim3(1), dim3(CLIP_WG), 0, st, nFiles, stride, d_payloadBytes, indexStride, d_indexBlocks, payloadCap, indexCap,
                       d_payloadOffs, d_indexOffs, d_outIndexBlocks, d_need);
    hipLaunchKernelGGL(k_corpus_copy, dim3(clip_grid(nFiles)), dim3(CLIP_WG), 0, st, nFiles, d_payload, stride, d_index, indexStride, d_outPayload, d_payloadOffs,
                       d_outIndex, d_indexOffs);
    CK(hipGetLastError());
    return ULCX_OK;
}
