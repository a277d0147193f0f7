// ulcx_rng_tables.h - host-side builder of the noise generator's jump and parity tables (UlcxDecCtx::jumpT / parT), shared
// by the library (ulcx_api.cpp) and the test-only unit module (ulcx_units.hip).  Not part of the public ABI.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

// Tables of the noise RNG (ulcDecoder.c:75-81).  xorshift32 is linear over GF(2): a matrix is kept as its 32 columns.
static uint32_t gf2_matvec(const uint32_t *col, uint32_t v) { uint32_t r = 0; for (int b = 0; b < 32; b++) if (v >> b & 1) r ^= col[b]; return r; }
static void gf2_matmul(uint32_t *out, const uint32_t *A, const uint32_t *Bm) { uint32_t t[32]; for (int b = 0; b < 32; b++) t[b] = gf2_matvec(A, Bm[b]); memcpy(out, t, sizeof(t)); }
static void build_rng_tables(std::vector<uint32_t> &jumpT) {
    auto step = [](uint32_t s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
    // jumpT[i][d][k][v]: byte k = v of the state, through T^(d * 16^i)
    jumpT.assign((size_t)8 * 16 * 4 * 256, 0u);
    uint32_t P[32];                                       // T^(16^i)
    for (int b = 0; b < 32; b++) P[b] = step(1u << b);
    for (int i = 0; i < 8; i++) {
        uint32_t Md[32];                                  // P^d
        for (int b = 0; b < 32; b++) Md[b] = 1u << b;
        for (int d = 1; d < 16; d++) {
            gf2_matmul(Md, P, Md);
            uint32_t *tab = jumpT.data() + ((size_t)(i * 16 + d) << 10);
            for (int k = 0; k < 4; k++)
                for (int v = 0; v < 256; v++) {
                    uint32_t r = 0;
                    for (int t = 0; t < 8; t++) if (v >> t & 1) r ^= Md[8 * k + t];
                    tab[k * 256 + v] = r;
                }
        }
        gf2_matmul(Md, P, Md);                            // P^16 = the next position's unit
        memcpy(P, Md, sizeof(P));
    }
    // parT[k][v][l] (round 5), appended: what lane l of the synthesis contributes to a unit's sign-parity stream, straight from
    // the unit's start state.  Bit i of the word = parity of the top bits of draws 32 l + 1 .. 32 l + i + 1 - linear in the
    // state, so it is (parity map) x T^(32 l), kept as four byte tables.  The start state is the same for all lanes of the wave:
    // with the LANE as the fastest index a look-up is one coalesced 256-byte row, not a gather.
    auto par_word = [&](uint32_t st) { uint32_t x = 0, par = 0; for (int i = 0; i < 32; i++) { st = step(st); par ^= st >> 31; x |= par << i; } return x; };
    uint32_t A[32], Ml[32];                               // A = T^32, Ml = A^l
    for (int b = 0; b < 32; b++) { uint32_t v = 1u << b; for (int i = 0; i < 32; i++) v = step(v); A[b] = v; Ml[b] = 1u << b; }
    const size_t base = jumpT.size();
    jumpT.resize(base + (size_t)4 * 256 * 64);
    for (int l = 0; l < 64; l++) {
        uint32_t col[32];
        for (int b = 0; b < 32; b++) col[b] = par_word(Ml[b]);
        for (int k = 0; k < 4; k++)
            for (int v = 0; v < 256; v++) {
                uint32_t r = 0;
                for (int t = 0; t < 8; t++) if (v >> t & 1) r ^= col[8 * k + t];
                jumpT[base + ((size_t)(k * 256 + v) << 6) + l] = r;
            }
        gf2_matmul(Ml, A, Ml);
    }
}
