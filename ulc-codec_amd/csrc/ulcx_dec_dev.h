// ulcx_dec_dev.h - the decoder's small pure device functions (ulcx_dec.hip), in a header so that the test-only unit
// module (ulcx_units.hip, tests/test_gpu_units.py) runs these very definitions.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
