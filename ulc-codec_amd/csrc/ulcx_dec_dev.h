// ulcx_dec_dev.h - the decoder's small pure device functions (ulcx_dec.hip), in a header so that the test-only unit
// module (ulcx_units.hip, tests/test_gpu_units.py) runs these very definitions.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ulcx_internal.h"

// ---------------------------------------------------------------------------
// The one view of a corpus (UlcxCorpus): file f of it, f inside [0, nFiles) by the caller's own test, and block k of that file.
// Neither the offset tables nor the index are trusted.  A ragged file whose offsets are negative, fall, leave their buffer, give a
// file of 2^31 bytes or more, or give a row without room for the file's indexBlocks + 1 entries is refused: ok false, nI = 0,
// avail = 0, and none of its bytes or entries is looked at.  A strided row's count is clamped so that its closing entry stays in the row,
// and its bytes to [0, payStride] (a negative payBytes fails every later comparison as it stands - avail is only ever the upper
// bound of an offset that is >= 0 -, so the clamp to 0 changes no result).
// ---------------------------------------------------------------------------
// bytes [p0, p1) of a buffer of `total` bytes as a file's payload (also k_dindex_ragged's test, which has no block count yet)
__device__ __forceinline__ bool corpus_bytes_ok(long long p0, long long p1, long long total) { return p0 >= 0 && p1 >= p0 && p1 <= total && p1 - p0 < 0x80000000LL; }
struct CorpusFile { const uint8_t *base; const ulcx_index_entry *row; long long avail; int nI; bool ok; };   // ok: not refused (row[0] exists)
// (ragged: s.payOffs != NULL, handed in so that a kernel compiled for one layout holds no code of the other)
__device__ __forceinline__ CorpusFile corpus_file(const UlcxCorpus &s, size_t f, bool ragged) {
    CorpusFile r;
    const int nI = s.indexBlocks[f];
    if (ragged) {
        const long long p0 = s.payOffs[f], p1 = s.payOffs[f + 1], i0 = s.idxOffs[f], i1 = s.idxOffs[f + 1];
        const bool okF = corpus_bytes_ok(p0, p1, s.payTotal) && i0 >= 0 && i1 >= i0 && i1 <= s.idxTotal && i1 - i0 > (long long)(nI < 0 ? 0 : nI);
        r.ok = okF; r.nI = okF ? (nI < 0 ? 0 : nI) : 0; r.avail = okF ? p1 - p0 : 0;
        r.base = s.pay + (okF ? p0 : 0); r.row = s.index + (okF ? i0 : 0);
    } else {
        r.ok = true; r.nI = (int)ulcx_row_blocks(nI, s.indexStride);
        const long long avail = s.payBytes[f];
        r.avail = avail < 0 ? 0 : avail > s.payStride ? s.payStride : avail;
        r.base = s.pay + f * (size_t)s.payStride; r.row = s.index + f * (size_t)s.indexStride;
    }
    return r;
}
// block k of the file: {byte offset in the file, bytes}; bytes 0 when there is none - k outside [0, nI), or bounding entries
// that are negative, do not rise or leave the file's bytes
struct FileBlock { int off, ext; };
__device__ __forceinline__ FileBlock file_block(const CorpusFile &f, long long k) {
    FileBlock b = { 0, 0 };
    if (k < 0 || k >= f.nI) return b;
    const long long o0 = f.row[k].ByteOffs, o1 = f.row[k + 1].ByteOffs;
    if (o0 < 0 || o1 <= o0 || o1 > f.avail) return b;
    b.off = (int)o0; b.ext = (int)(o1 - o0);
    return b;
}

// ---------------------------------------------------------------------------
__device__ __forceinline__ float expand_quantizer(int q) {        // ulcDecoder.c:96-98
    return 0x1.0p-31f * (float)((1u << (31 - 5)) >> q);
}
__host__ __device__ constexpr uint32_t xorshift32(uint32_t s) {    // ulcDecoder.c:75-81
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return s;
}
// ---------------------------------------------------------------------------
// One whole code of the block syntax (FormatSpecs.md:57-141, ulcDecoder.c:99-197) decoded from a
// 32-bit window (>= 7 nybbles, low nybble first), with selects instead of a branch cascade:
// every lane of a wave executes the same instruction stream whatever its own code is.
//   plain  +-2..+-7          1 nybble   one coefficient
//   0h,X                     2          X+1 zeros
//   1h,Y,X                   3          YX+33 zeros
//   8h,Z,Y,X                 4          noise run: n = (ZY<<1 | X&1) + 16, level (X>>1)+1
//   Fh,X (X < Eh)            2          quantizer X
//   Fh,Eh,X (X < Fh)         3          quantizer Eh+X;  Fh,Eh,Fh = stop (zeros to the end)
//   Fh,Fh,Z,Y,X              5          noise to the end: level Z+1, decay YX
// A unit opens with a quantizer code without its Fh prefix (`first`); a leading Fh there (only a corrupt
// stream has one) gives the quantizer 0.0 the reference computes for it.
// ---------------------------------------------------------------------------
struct Code {
    int len;            // nybbles
    int n;              // coefficients consumed at once (1, or a zero run)
    int np;             // noise coefficients of a run (tail: the caller uses N)
    int l, dn, sv;      // noise level / tail decay / signed square of a plain coefficient
    int qnew;           // new quantizer index or -1
    int plain, zrun, n8, tail, stop;     // 0 / 1
};
// Classification by bit tests on constants indexed with the nybble, and arithmetic on the 0/1 results: written with
// comparisons (v0 == 0, == 1, == 8, == Fh ...) the compiler recognises a switch and lowers it to a tree of branches with
// EXEC-mask bookkeeping - in a kernel whose every instruction costs a wave ~9 cycles.
__device__ __forceinline__ Code decode_code(uint32_t w, bool first) {
    Code k;
    const int f = first ? 1 : 0;
    const int q15 = f & (int)(((w & 0xF) + 1) >> 4);
    w = first ? ((w << 4) | 0xF) : w;
    const int v0 = w & 0xF, v1 = (w >> 4) & 0xF, v2 = (w >> 8) & 0xF, v3 = (w >> 12) & 0xF, v4 = (w >> 16) & 0xF;
    const int z0 = (0x0001 >> v0) & 1, z1 = (0x0002 >> v0) & 1, esc = (0x8000 >> v0) & 1;
    k.n8 = (0x0100 >> v0) & 1;
    k.plain = (0x7EFC >> v0) & 1;
    k.zrun = (0x0003 >> v0) & 1;
    k.tail = esc & ((v1 + 1) >> 4) & (q15 ^ 1);
    const int qext = esc & ((0x4000 >> v1) & 1);
    k.stop = qext & ((v2 + 1) >> 4);
    const int q1 = esc & (k.tail ^ 1) & (qext ^ 1);
    const int sgn = (v0 ^ 0x8) - 0x8;
    const int sq = sgn * sgn;
    k.sv = (sgn < 0) ? -sq : sq;
    // nybbles: 1 plain, 2 short zero run, 3 long zero run, 4 noise run; Fh: 2, +1 quantizer extension / stop, +3 tail
    const int len0 = (int)((0x2111111411111132ull >> (4 * v0)) & 0xF);
    k.len = len0 + 3 * k.tail + qext - f;
    const int v12 = (v1 << 4) | v2;
    k.n = k.plain + z0 * (v1 + 1) + z1 * (v12 + 33);
    k.np = k.n8 * (((v12 << 1) | (v3 & 1)) + 16);
    k.l = (v2 + 1) + k.n8 * ((v3 >> 1) - v2);
    k.dn = (v3 << 4) | v4;
    // (opening Fh: the reference expands quantizer -2, ulcDecoder.c:89-98,107 - a shift by -2, i.e. by 30 on x86-64:
    //  the unit's quantizer is exactly 0 until a change code; index 30 expands to the same 0)
    const int qn = -1 + q1 * (v1 + 1) + (qext & (k.stop ^ 1)) * (0xE + v2 + 1);
    k.qnew = q15 ? 30 : qn;
    return k;
}
// number of leading nybbles of w (low first, at most 7) that are plain coefficients, i.e. none of 0h 1h 8h Fh
__device__ __forceinline__ int plain_prefix(uint32_t w) {
    auto zn = [](uint32_t x) { return (x - 0x11111111u) & ~x & 0x88888888u; };       // bit 3 of every nybble that is 0 (exact for the lowest such nybble)
    uint32_t sp = zn(w) | zn(w ^ 0x11111111u) | zn(w ^ 0x88888888u) | zn(w ^ 0xFFFFFFFFu);
    sp |= 0x80000000u;                                   // the 8th nybble is not part of the window
    return (__ffs((int)sp) - 1) >> 2;                    // index of the first special nybble
}

// ---------------------------------------------------------------------------
// xorshift32 is linear over GF(2): the state after n draws is T^n * state.  jumpT holds T^(d*16^i) for every
// hexadecimal digit d of n at every position i, each as four 256-entry byte tables (host-built, ulcx_rng_tables.h):
// a jump costs one table-driven mat-vec (4 lookups) per non-zero digit.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rng_jump(const uint32_t *__restrict__ jt, uint32_t s, uint32_t n) {
    for (int i = 0; n; i++, n >>= 4) {
        const uint32_t dgt = n & 15u;
        if (dgt) {
            const uint32_t *J = jt + ((size_t)(i * 16 + dgt) << 10);
            s = J[s & 255u] ^ J[256 + ((s >> 8) & 255u)] ^ J[512 + ((s >> 16) & 255u)] ^ J[768 + (s >> 24)];
        }
    }
    return s;
}

// wave-wide inclusive prefix sum / prefix maximum of one 32-bit value per lane (row shifts + row broadcasts)
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    return v;
}
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
    v = umax32(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
    return v;
}

// ---------------------------------------------------------------------------
// Output samples.  OUT = float: the C API's layout; OUT = int16_t: PCM16 output, converted on store
// exactly as the reference's WAV writer does (tools/WavIO_Helper.c:9-13,56-63: lrintf(clamp(x * 2^15, -32768, 32767))).
__device__ __forceinline__ int16_t to_pcm16(float x) {
    float v = x * 0x1.0p+15f;
    v = (v < -32768.0f) ? -32768.0f : (v > 32767.0f) ? 32767.0f : v;
    return (int16_t)__float2int_rn(v);
}
