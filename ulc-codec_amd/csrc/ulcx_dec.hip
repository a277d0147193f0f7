// ulcx_dec.hip — batched ulc-codec decoder for gfx950 (MI355X), hand-written HIP.
//
// Two kernels per call; dequantised coefficients never exist in HBM:
//   k_dscan   one lane per block: the serial syntax walk (libulc/ulcDecoder.c:99-197, syntax
//             FormatSpecs.md:57-141).  It is the one thing that cannot be done in parallel, so it does
//             nothing but walk and take notes: 8-byte records of the runs of coded coefficients and of
//             the noise runs (about 1 KB per block instead of 16 KB of coefficients), RNG draw counts,
//             and the decaying-noise level chain of each unit's tail.
//   k_dscan_rows  the same walk for every call that finds its blocks through a block index (range calls, crops of a strided or
//             ragged corpus, sample crops, spectra): one lane per (row, block), the row's file and the block's extent through the
//             one view of a corpus (UlcxCorpus; corpus_file / file_block in ulcx_dec_dev.h), which the splice kernels share.
//   k_dsyn    stereo streams: one workgroup (2 waves) per stream, blocks in order, one wave per channel:
//             the records are scattered STRAIGHT INTO the FFT's LDS arrays, noise runs are synthesised
//             32 coefficients per lane from a jumped-ahead xorshift state (top bits by parity masks), then
//             IMDCT (one DCT-IV = complex FFT per channel, one wave per array, no barrier between the
//             passes), sine-window overlap-add, the centring of decimated subblocks on one timeline
//             (the reference's reversed-time FIFO without the shifting: dec_time_wave), inverse M/S,
//             interleave (libulc/ulcDecoder.c:198-302; IMDCT per FormatSpecs.md:150-157).
//   k_dgen    every other geometry (mono, multichannel, BlockSize > 4096): same pieces, one array.
//   k_dspec   spectra calls (ulcx_decode_crops_spectra_*): in place of the synthesis - the dequantised coefficients themselves,
//             one workgroup per (row, block, channel pair), stored channels-first; the one call whose coefficients do reach HBM.
//   k_ddist   distortion calls (ulcx_decode_crops_distortion_*): k_dspec's grid and expansion, and in place of its stores binary64
//             sums of the coefficients against caller-held reference planes, per segment of the block, in one fixed order.
// Compiled with -ffp-contract=off (see ulcx_enc.hip).
#include "ulcx_internal.h"
#include "ulcx_dec_dev.h"

#define WG 128
#define FFT_PACKED
#include "ulcx_fft.h"
#define DSYN_TWL ULCX_DSYN_TWL
// Settled by measurement: each line names the note that holds the alternative's numbers.
#define DSYN_C2048 1   // BlockSize 2048 as a compile-time constant of k_dsyn (0: read from the context; profiles/NOTES_r01-r04.md)
#define DSYN_C4096 1   // BlockSize 4096 likewise, with the pipelined epilogue (profiles/NOTES_r05.md)
#define DSYN_EPI2 1    // those two: the epilogue's global operands fetched one trip ahead (0: the generic loop; profiles/NOTES_r05.md)
#define DPS 4          // FFT array padding (ulcx_fft.h): one complex after every 16 (3: after every 8 - conflict-free passes, 1 KB more LDS; profiles/NOTES_r01-r04.md)

// ---------------------------------------------------------------------------
// The scan's view of the stream: 16-byte aligned chunks kept in registers, the next one always in flight, so a
// trip of the walk waits for memory once per 32 nybbles instead of once per code.
// ---------------------------------------------------------------------------
struct NybWin {
    const uint8_t *p16;          // 16-byte aligned address at or below the block's first byte
    int a;                       // bytes between p16 and the block's first byte
    int readBytes;               // block bytes that may be used (later ones read as 0)
    const uint8_t *bufBeg, *bufEnd;   // the caller's whole input: nothing outside it is touched
    uint32_t c0, c1, c2, c3, n0, n1, n2, n3; int chunk;       // current and next 16-byte chunk (scalars: a struct member picked
                                                              // by a run-time index makes the compiler move the window to LDS)

    __device__ __forceinline__ void load_chunk(int ci, uint32_t &o0, uint32_t &o1, uint32_t &o2, uint32_t &o3) const {
        const uint8_t *q = p16 + (ptrdiff_t)ci * 16;
        const int rel = ci * 16 - a;                       // block-relative offset of the chunk's first byte
        uint32_t d0, d1, d2, d3;
        if (q >= bufBeg && q + 16 <= bufEnd) { const uint4 v = *(const uint4 *)q; d0 = v.x; d1 = v.y; d2 = v.z; d3 = v.w; }
        else {
            auto word = [&](int j) { uint32_t w = 0; for (int t = 0; t < 4; t++) { const uint8_t *b = q + 4 * j + t; if (b >= bufBeg && b < bufEnd) w |= (uint32_t)*b << (8 * t); } return w; };
            d0 = word(0); d1 = word(1); d2 = word(2); d3 = word(3);
        }
        if (rel + 16 > readBytes) {
            auto mask = [&](int j) { const int keep = readBytes - (rel + 4 * j); return keep >= 4 ? 0xFFFFFFFFu : keep <= 0 ? 0u : ((1u << (8 * keep)) - 1u); };
            d0 &= mask(0); d1 &= mask(1); d2 &= mask(2); d3 &= mask(3);
        }
        o0 = d0; o1 = d1; o2 = d2; o3 = d3;
    }
    __device__ __forceinline__ void init(const uint8_t *p, int rb, const uint8_t *b0, const uint8_t *b1) {
        a = (int)((uintptr_t)p & 15); p16 = p - a; readBytes = rb; bufBeg = b0; bufEnd = b1;
        chunk = 0; load_chunk(0, c0, c1, c2, c3); load_chunk(1, n0, n1, n2, n3);
    }
    __device__ __forceinline__ void advance(int q) {
        if ((q >> 5) > chunk) { c0 = n0; c1 = n1; c2 = n2; c3 = n3; chunk++; load_chunk(chunk + 1, n0, n1, n2, n3); }
    }
    // window at bit position pos of the block (positions only ever advance, by at most 12 nybbles per call)
    __device__ __forceinline__ uint32_t at(int pos) {
        const int q = (pos >> 2) + 2 * a;
        advance(q);
        const int di = (q >> 3) & 3, sh = (q & 7) * 4;
        uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = n0;
        asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4));
        const uint32_t lo = di == 0 ? x0 : di == 1 ? x1 : di == 2 ? x2 : x3;
        const uint32_t hi = di == 0 ? x1 : di == 1 ? x2 : di == 2 ? x3 : x4;
        return __builtin_amdgcn_alignbit(hi, lo, sh);
    }
    // the same, 64 bits wide: a trip's run of plain nybbles (<= 28 bits) and the code behind it (<= 20 bits) from one look
    __device__ __forceinline__ uint64_t at64(int pos) {
        const int q = (pos >> 2) + 2 * a;
        advance(q);
        const int di = (q >> 3) & 3, sh = (q & 7) * 4;
        // (values first, opaque to the optimiser, then selects: a select between loads of struct members becomes a load from
        //  a selected address, and a window that is indexed at run time is moved to LDS - one LDS round trip per trip)
        uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = n0, x5 = n1;
        asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5));
        const uint32_t d0 = di == 0 ? x0 : di == 1 ? x1 : di == 2 ? x2 : x3;
        const uint32_t d1 = di == 0 ? x1 : di == 1 ? x2 : di == 2 ? x3 : x4;
        const uint32_t d2 = di == 0 ? x2 : di == 1 ? x3 : di == 2 ? x4 : x5;
        return (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32);
    }
};

// The same view for a lane whose every look stays inside the caller's buffer (k_dscan checks that per wave: all but the
// waves at the buffer's ends), without NybWin's stall: there the load sits in a branch and its result is copied into the
// loop-carried registers right behind it, so the compiler waits for it on the spot (`s_waitcnt vmcnt(0)`, records stored
// since included) - a memory round trip in almost every trip of a wave, some lane of 64 always being at a chunk's end.
// Here every look issues ONE load into registers nothing touches before the next look (a trip of the walk is ~1500
// cycles of dependent arithmetic: a chunk's latency): a lane that moved on to its next chunk fetches the chunk two
// ahead, every other lane reads one common address (one line for all of them), and the next look takes the value over
// with a select.  The shift to the next chunk is a select too.
// Bytes behind readBytes are not masked: limit = 8 readBytes in every caller, a code that uses a nybble behind it ends
// behind limit, and the walk calls that block corrupt whatever the nybble was.
struct NybWinFast {
    const uint4 *p16, *common; int a; int chunk; bool gNew;
    uint32_t c0, c1, c2, c3, n0, n1, n2, n3, f0, f1, f2, f3, g0, g1, g2, g3;
    __device__ __forceinline__ void init(const uint8_t *p, int, const uint8_t *, const uint8_t *) {
        a = (int)((uintptr_t)p & 15); p16 = (const uint4 *)(p - a); chunk = 0; gNew = false;
        common = (const uint4 *)(((uintptr_t)__builtin_amdgcn_readfirstlane((int)((uintptr_t)p16 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uintptr_t)p16));
        const uint4 v0 = p16[0], v1 = p16[1], v2 = p16[2];
        c0 = v0.x; c1 = v0.y; c2 = v0.z; c3 = v0.w; n0 = v1.x; n1 = v1.y; n2 = v1.z; n3 = v1.w; f0 = v2.x; f1 = v2.y; f2 = v2.z; f3 = v2.w;
        g0 = g1 = g2 = g3 = 0;
    }
    __device__ __forceinline__ uint64_t at64(int pos) {
        const int q = (pos >> 2) + 2 * a;
        f0 = gNew ? g0 : f0; f1 = gNew ? g1 : f1; f2 = gNew ? g2 : f2; f3 = gNew ? g3 : f3;      // the last look's load
        const bool adv = (q >> 5) > chunk;                   // (a trip moves at most 12 nybbles: one chunk at a time)
        c0 = adv ? n0 : c0; c1 = adv ? n1 : c1; c2 = adv ? n2 : c2; c3 = adv ? n3 : c3;
        n0 = adv ? f0 : n0; n1 = adv ? f1 : n1; n2 = adv ? f2 : n2; n3 = adv ? f3 : n3;
        chunk += adv ? 1 : 0;
        const uint4 v = *(adv ? p16 + (chunk + 2) : common);
        g0 = v.x; g1 = v.y; g2 = v.z; g3 = v.w; gNew = adv;
        const int di = (q >> 3) & 3, sh = (q & 7) * 4;
        uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = n0, x5 = n1;
        asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5));
        const uint32_t d0 = di == 0 ? x0 : di == 1 ? x1 : di == 2 ? x2 : x3;
        const uint32_t d1 = di == 0 ? x1 : di == 1 ? x2 : di == 2 ? x3 : x4;
        const uint32_t d2 = di == 0 ? x2 : di == 1 ? x3 : di == 2 ? x4 : x5;
        return (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32);
    }
    __device__ __forceinline__ uint32_t at(int pos) { return (uint32_t)at64(pos); }
};

// Where the walk's records go (k_dscan).  Every lane appends 8-byte records to the row of ITS block: stored one by one
// that is up to 64 partial lines per store instruction and two such instructions per trip - more than half of the
// kernel's time, and three times the records' bytes in HBM traffic (partly written lines evicted and fetched again).
// Instead a lane parks its records in an LDS ring (row r of the ring holds the records number r mod R of every lane, rotated
// by r so that one lane's consecutive records lie in different banks), and when some lane's ring is nearly full the
// wave writes out all of them: two owners per trip, a half-wave per owner, the owner's pending records to consecutive
// addresses of its row.
#define DSCAN_RP 24              // plain-run records a lane may have pending (a trip adds at most two)
#define DSCAN_RN 12              // noise records (at most one per trip)
#define DSCAN_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
template <int R>
__device__ __forceinline__ void ring_put(uint2 *ring, int lane, int slotR, uint2 rec) { ring[slotR * 64 + ((lane + slotR) & 63)] = rec; }
// f .. n-1: this lane's pending records; rowIdx: its block; base + rowIdx * stride: the block's row (stride records)
template <int R>
__device__ __forceinline__ void ring_flush(uint2 *ring, int lane, int &f, int n, uint2 *base, int rowIdx, int stride) {
    DSCAN_WAVE_SYNC();
    const int cnt = n - f, half = lane >> 5, i = lane & 31;
    const unsigned long long pend = __ballot(cnt > 0);       // (a wave with few live lanes - the drop-in's one block - skips the rest)
#pragma unroll 4
    for (int it = 0; it < 32; it++) {
        if (!((pend >> (2 * it)) & 3ull)) continue;
        const int j = 2 * it + half;
        const int cj = __builtin_amdgcn_ds_bpermute(j << 2, cnt);
        const int fj = __builtin_amdgcn_ds_bpermute(j << 2, f);
        const int rj = __builtin_amdgcn_ds_bpermute(j << 2, rowIdx);
        const int idx = fj + i;
        const int r = idx % R;
        if (i < cj && idx < stride) base[(size_t)rj * stride + idx] = ring[r * 64 + ((j + r) & 63)];
    }
    f = n;
    DSCAN_WAVE_SYNC();
}

// A block's shape from its window code: the subblock pattern (a nybble per subblock, ulcx_pattern; code 0000 behaves as one
// plain N/1 block, as in the reference), the subblocks per channel, and whether that is the one full-size subblock
// (ulcDecoder.c:242-245).
struct BlockShape { unsigned pat; int nsub; bool whole; };
__device__ __forceinline__ BlockShape block_shape(int BS, int wc) {
    BlockShape b;
    b.pat = ulcx_pattern(wc);
    b.whole = (BS >> (b.pat & 7)) == BS;
    b.nsub = 1;
    if (!b.whole) { b.nsub = 0; unsigned q = b.pat; do b.nsub++; while (q >>= 4); }
    return b;
}
// LastSubBlockSize as a block with this window code leaves it (ulcDecoder.c:300): the size of its last subblock
__device__ __forceinline__ int last_sub_size(int BS, int wc) {
    const unsigned pat = ulcx_pattern(wc);
    unsigned pp = pat; int ls = BS;
    if ((BS >> (pat & 7)) != BS) do { ls = BS >> (pp & 7); } while (pp >>= 4);
    return ls;
}
// Windowed overlap-add of one pair (spec v2, oracle/orc_fourier.c orc_imdct): A the pending sample, B the new one, (cw, sn) the
// window's falling and rising value at the pair.  Out[p] = fma(c, A, -(s B)), Out[S-1-p] = fma(s, A, c B) - the products
// rounded on their own, as the reference writes them; below the ramp (pass) both go through unchanged.
struct LapPair { float lo, hi; };
__device__ __forceinline__ LapPair lap_pair(float A, float B, float cw, float sn, bool pass) {
    LapPair r;
    if (pass) { r.lo = A; r.hi = B; }
    else {
        const float m1 = sn * B, m3 = cw * B;
        r.lo = __builtin_fmaf(cw, A, -m1); r.hi = __builtin_fmaf(sn, A, m3);
    }
    return r;
}

// Syntax walk of one block starting at p (limit = bits that may be consumed, readBytes = bytes that may be
// used).  The walk is the one thing that cannot be done in parallel; everything it learns on the way is left for the
// synthesis in a form that can: per (channel, subblock) unit
//   * PLAIN-RUN records, 8 bytes: up to seven consecutive coded coefficients {first coefficient | quantizer index << 15 |
//     count << 20, their nybbles};
//   * NOISE records, 8 bytes (the layout synth_noise reads): {first coefficient | count << 16 | tail << 31,
//     draws made in the unit before the run | level << 16 | quantizer index << 21};
//   * the unit's draws-so-far, its decaying-noise tail's parameters and (after the walk) the tail's level chain;
// and bits / WindowCtrl / draws of the block.  One flat loop, one code (or one
// run of plain coefficients) per trip.
// RING: the records through the wave's LDS rings (every lane of the wave is here, `live` or not, and stays to the end);
// else stored one by one (lanes come and go as they please: k_dscan_packed).
// NOTES = false (k_dindex): the same walk and NOTHING stored - no records, no per-unit or per-block notes, no tail chains;
// blk is not looked at.  What the walk hands back either way: the bits consumed (0 = corrupt) and the block's draws.
struct Walked { int bits, draws; };
template <typename WIN = NybWin, bool RING = false, bool NOTES = true>
__device__ __forceinline__ Walked scan_block(const UlcxDecCtx &c, int blk, const uint8_t *p, int limit, int readBytes,
                                             const uint8_t *bufBeg, const uint8_t *bufEnd, bool live = true, uint2 *ringP = nullptr, uint2 *ringN = nullptr) {
    static_assert(NOTES || !RING, "scan_block: the rings carry records");
    const int rlane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    int fP = 0, fN = 0, wP = 0, wN = 0;                             // RING: records written out so far, ring rows of the next records
    WIN win; win.init(p, readBytes, bufBeg, bufEnd);
    int pos = 0;
    int wc;
    {
        uint32_t w0 = (limit >= 8) ? win.at(0) : 0;                 // ulcDecoder.c:211-216
        wc = w0 & 0xF;
        bool dec = (wc & 0x8) != 0;
        wc |= dec ? (int)(w0 & 0xF0) : (1 << 4);
        pos = dec ? 8 : 4;
    }
    // (block_shape, written out: with the helper's branch on `whole` the three scans grow by 16-36 bytes)
    unsigned pat = ulcx_pattern(wc);                                // (code 0000 behaves as one plain N/1 block, as in the reference)
    int nsub = 0; { unsigned q = pat; do nsub++; while (q >>= 4); }
    if ((c.BS >> (pat & 7)) == c.BS) nsub = 1;                      // ulcDecoder.c:242-245
    int total = c.C * nsub;
    // the block's rows of the per-block scratch: addresses only - every access sits under NOTES (k_dindex walks more blocks
    // than the scratch has rows)
    int *udraw  = c.unitDraws + (size_t)blk * c.C * 4;
    int4 *urec = c.unitRec + (size_t)blk * c.C * 4;
    float4 *utail = c.unitTail + (size_t)blk * c.C * 4;
    uint2 *prec = c.prec + (size_t)blk * c.precStride;
    uint2 *nrec = c.nrec + (size_t)blk * c.nrecStride;
    int nP = 0, nN = 0, uP0 = 0, uN0 = 0;                           // records written so far in the block / at the current unit's start
    auto put_prec = [&](uint2 rec) {
        if constexpr (NOTES) {
            if (RING) { ring_put<DSCAN_RP>(ringP, rlane, wP, rec); wP = (wP + 1 == DSCAN_RP) ? 0 : wP + 1; }
            else if (nP < c.precStride) prec[nP] = rec;
            nP++;
        }
    };
    auto put_nrec = [&](uint2 rec) {
        if constexpr (NOTES) {
            if (RING) { ring_put<DSCAN_RN>(ringN, rlane, wN, rec); wN = (wN + 1 == DSCAN_RN) ? 0 : wN + 1; }
            else if (nN < c.nrecStride) nrec[nN] = rec;
            nN++;
        }
    };
    int u = 0, draws = 0, uslot = 0, uDraw0 = 0, uj = 0, uch4 = 0;
    if constexpr (NOTES) { if (live) { udraw[0] = 0; utail[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); } }
    int S = c.BS >> (pat & 7), N = S;
    bool first = true;
    bool fin = (limit < 16) | !live, bad = fin;
    auto next_unit = [&]() {
        if constexpr (NOTES) urec[uslot] = make_int4(uP0, nP - uP0, uN0, nN - uN0);
        u++;
        fin = bad | (u >= total);
        if (!fin) {
            uj++;                                                  // (subblock within the channel, channel * 4: counters, not a division by nsub)
            if (uj == nsub) { uj = 0; uch4 += 4; }
            const int j = uj;
            uslot = uch4 + j;
            if constexpr (NOTES) udraw[uslot] = draws;
            uDraw0 = draws;
            if constexpr (NOTES) utail[uslot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uP0 = nP; uN0 = nN;
            S = c.BS >> ((pat >> (4 * j)) & 7); N = S;
            first = true;
        }
    };
    int qidx = 30;                                                  // (index 30 expands to 0.0; every unit opens with a quantizer code)
    // One trip = a run of plain coefficient nybbles (possibly empty), then ONE other code: every lane does both parts every
    // trip, so lanes that alternate between the two kinds (the usual stream) do not wait for each other's other half.
    for (;;) {
        if (RING) { if (!__any(!fin)) break; } else if (fin) break;
        if (!fin) {
        const uint64_t w64 = win.at64(pos);
        uint32_t w = (uint32_t)w64;
        // 1. plain coefficients (+-2..+-7), up to the seven the window holds.  Never across the unit end or the block's bits;
        //    not at a unit's opening code.
        int m = first ? 0 : plain_prefix(w);
        m = m < N ? m : N;
        m = (pos + 4 * m <= limit) ? m : 0;
        if (m > 0) {
            put_prec(make_uint2((uint32_t)(S - N) | ((uint32_t)qidx << 15) | ((uint32_t)m << 20), w & (0xFFFFFFFFu >> (32 - 4 * m))));
            pos += 4 * m; N -= m;
            if (N == 0) next_unit();
            w = (uint32_t)(w64 >> (4 * m));
        }
        if (!fin) {
        // 2. one code
        Code k = decode_code(w, first);
        const bool over = (k.zrun & (k.n > N)) | (k.n8 & (k.np > N));     // ulcDecoder.c:127,139,154
        const bool toEnd = k.stop | k.tail;
        const int used = over ? 0 : (toEnd ? N : k.n + k.np);
        qidx = (k.qnew >= 0) ? k.qnew : qidx;                              // ulcDecoder.c:89-98
        if (k.plain) put_prec(make_uint2((uint32_t)(S - N) | ((uint32_t)qidx << 15) | (1u << 20), w & 0xFu));   // (a plain coefficient part 1 left: the block's bits end inside the run)
        if ((k.n8 | k.tail) & !over) {
            const int np = k.tail ? N : k.np;
            put_nrec(make_uint2((uint32_t)(S - N) | ((uint32_t)(np - (k.tail ? 1 : 0)) << 16) | (k.tail ? 0x80000000u : 0u),
                                (uint32_t)(draws - uDraw0) | ((uint32_t)k.l << 16) | ((uint32_t)qidx << 21)));
        }
        if constexpr (NOTES) if (k.tail & !over) {
            // ulcDecoder.c:163-186: start amplitude, decay, first coefficient, count; the chain itself runs after the walk
            const float lev0 = (float)(k.l * k.l) * expand_quantizer(qidx) * (1.0f / 16);
            const float rr = 1.0f + (float)(k.dn * k.dn) * -0x1.0p-19f;
            utail[uslot] = make_float4(lev0, rr, __int_as_float(S - N), __int_as_float(N));
        }
        draws += over ? 0 : (k.tail ? N : k.np);
        pos += 4 * k.len;
        N -= used;
        bad |= over;
        first = false;
        if ((N == 0) | over) next_unit();
        if (pos > limit) { bad = true; fin = true; }               // ran off the readable bytes: corrupt
        }
        }
        if (RING && __any((nP - fP > DSCAN_RP - 2) | (nN - fN > DSCAN_RN - 1))) {
            ring_flush<DSCAN_RP>(ringP, rlane, fP, nP, c.prec, blk, c.precStride);
            ring_flush<DSCAN_RN>(ringN, rlane, fN, nN, c.nrec, blk, c.nrecStride);
        }
    }
    if (RING) {
        ring_flush<DSCAN_RP>(ringP, rlane, fP, nP, c.prec, blk, c.precStride);
        ring_flush<DSCAN_RN>(ringN, rlane, fN, nN, c.nrec, blk, c.nrecStride);
        if (!live) return Walked{ 0, 0 };
    }
    bool ok = !bad;
    if constexpr (NOTES) {
    c.bits[blk] = ok ? pos : 0;
    c.wcScan[blk] = ok ? wc : 0;
    c.draws[blk] = draws;
    // Decaying-noise tails (ulcDecoder.c:176-186: v = p; p *= r per coefficient): the magnitude chain is one serial
    // float recurrence per unit.  It runs here, 64 units abreast, and leaves the magnitude at every 32nd coefficient
    // position so that the synthesis can start anywhere.
    if (ok) {
        for (int t = 0; t < total; t++) {
            int ch = t / nsub, j = t - ch * nsub, us = ch * 4 + j;
            float4 tp = utail[us];
            int n = __float_as_int(tp.w);
            if (n <= 0) continue;
            int p0 = __float_as_int(tp.z);
            float lev = tp.x; const float rr = tp.y;
            float *tm = c.tailMag + ((size_t)blk * c.C * 4 + us) * c.tailStride;
            int i = p0, end = p0 + n;
            while (i < end && (i & 31)) { lev *= rr; i++; }        // up to the first chunk boundary
            for (; i < end; i += 32) {
                tm[i >> 5] = lev;
#pragma unroll
                for (int q = 0; q < 32; q++) lev *= rr;
            }
        }
    }
    }
    return Walked{ ok ? pos : 0, draws };
}

// Pass 1 - one lane per block.
__global__ __launch_bounds__(64) void k_dscan(UlcxDecCtx c) {
    __shared__ uint2 ringP[DSCAN_RP * 64], ringN[DSCAN_RN * 64];
    const int id0 = blockIdx.x * 64 + threadIdx.x, Kc = c.k1 - c.k0;      // streams [s0, s1), blocks [k0, k1) of each
    const bool live = id0 < (c.s1 - c.s0) * Kc;
    const int id = live ? id0 : (c.s1 - c.s0) * Kc - 1;                   // (a lane without a block shadows the last one, and writes nothing)
    const int blk = (c.s0 + id / Kc) * c.K + c.k0 + id % Kc;
    const uint8_t *p = c.in + (size_t)blk * c.slot, *bufEnd = c.in + c.inBytes;
    // every look of every lane of the wave inside the buffer (a look reads up to three 16-byte chunks behind the one
    // the position is in, and the position stops at the slot's end): the window without bounds checks
    const bool inside = (size_t)(p - c.in) >= ((uintptr_t)p & 15) && (size_t)(bufEnd - p) >= (size_t)c.slot + 80;
    if (__ballot(!inside) == 0ull) scan_block<NybWinFast, true>(c, blk, p, c.slot * 8, c.slot, c.in, bufEnd, live, ringP, ringN);
    else scan_block<NybWin, true>(c, blk, p, c.slot * 8, c.slot, c.in, bufEnd, live, ringP, ringN);
}

// Pass 1, packed payloads - one lane per stream: a block's start is only known once the previous
// block has been parsed (the container stores no block lengths, tools/ulcDecodeTool.c:153-165).
__global__ __launch_bounds__(64) void k_dscan_packed(UlcxDecCtx c) {
    int s = c.s0 + blockIdx.x * 64 + threadIdx.x;
    if (s >= c.s1) return;
    int off = c.packOff[s];
    int avail = c.payBytes[s];
    const uint8_t *base = c.in + (size_t)s * c.payStride;
    bool dead = false;
    for (int k = 0; k < c.K; k++) {
        int blk = s * c.K + k;
        c.blkOff[blk] = off;
        int bits = 0;
        if (!dead && off < avail) bits = scan_block(c, blk, base + off, (avail - off) * 8, avail - off, c.in, c.in + c.inBytes).bits;
        else { c.bits[blk] = 0; c.wcScan[blk] = 0; c.draws[blk] = 0; }
        if (!bits) dead = true;
        off += (bits + 7) >> 3;                                     // the tool rounds every block up to a byte
    }
    c.packOff[s] = off;
}

// Pass 1 of every call that finds its blocks through a block index - one lane per (row, block-row), as k_dscan: the index gives
// every block's start and its exact extent, so nothing is walked in series.  Row r of row-of-the-call i is block rFirst[i] - 1 + r
// of the row's file (row 0: the block in front, run without output for the lapping state), found through the one view of the
// corpus (corpus_file / file_block).  The two kinds of call differ in four things, each picked by `crop` (one kernel with uniform
// branches: compiled once for each kind, the range call's scan stage measured 2 % longer, profiles/corpus_view_ab.txt):
//   a range call (ulcx_decode_range_*, file == NULL): the corpus is the decoder's own streams and row i is stream i; every block
//     of the row is wanted; a row stays sane block by block (an entry that points outside its stream's payload marks that block
//     alone); and the packed read position behind the range is written (the closing entry when the range runs past the
//     stream's end: where a sequential decode stops).
//   a crop call (ulcx_decode_crops_*): row i names file file[i] of a corpus, strided or ragged, that is looked at only once the
//     number is known to lie inside [0, nFiles), and any number of rows may name one file; count[i] leading blocks are wanted, or
//     all; a row is all or nothing (below); no read position is written - a crop belongs to no stream.
// A lane without a block - a file or a start out of range, a block in front of block 0, at or past the file's block count or
// the row's count, a refused file or entry - marks it as a corrupt block is (window code 0: the row ends there).
__global__ __launch_bounds__(64) void k_dscan_rows(UlcxDecCtx c, UlcxCorpus cp, const int32_t *file, const int32_t *count) {
    __shared__ uint2 ringP[DSCAN_RP * 64], ringN[DSCAN_RN * 64];
    const int id0 = blockIdx.x * 64 + threadIdx.x, K = c.K;
    const bool live0 = id0 < c.B * K, crop = file != nullptr;
    const int id = live0 ? id0 : c.B * K - 1;                             // (a lane without a row shadows the last one, and writes nothing)
    const int s = id / K, r = id - s * K;
    const int f = crop ? file[s] : s;
    const bool okF = f >= 0 && f < cp.nFiles;
    const CorpusFile cf = corpus_file(cp, okF ? (size_t)f : 0, cp.payOffs != nullptr);           // (nFiles >= 1: file 0 exists, and nothing of it is used for a bad row)
    const int nI = cf.nI, first = c.rFirst[s];
    int want = count ? count[s] : K - 1;                                  // leading blocks of the row that are wanted (K >= 2)
    want = want > K - 1 ? K - 1 : want;
    bool okS = okF && cf.ok && first >= 0 && first <= nI && want > 0;
    if (okS && crop) {
        // the table is not trusted, and a crop row is all or nothing: every entry that bounds a block of the row (the one in front
        // included) inside the file's payload and behind its predecessor - each lane looks at its row's <= K + 1 entries
        const int j0 = first > 0 ? first - 1 : 0, j1 = first + want < nI ? first + want : nI;
        long long prev = cf.row[j0].ByteOffs;
        bool okT = prev >= 0;
        for (int j = j0 + 1; j <= j1; j++) { const long long o = cf.row[j].ByteOffs; okT &= o > prev && o <= cf.avail; prev = o; }
        okS = okT;
    }
    FileBlock b = { 0, 0 };
    if (okS && r <= want) b = file_block(cf, first - 1 + r);
    const bool sane = b.ext > 0;
    const int ext = b.ext;
    const uint8_t *p = cf.base + b.off, *bufEnd = cp.pay + cp.payTotal;
    // every look of every lane of the wave inside the buffer (k_dscan): the window without bounds checks
    const bool inside = (size_t)(p - cp.pay) >= ((uintptr_t)p & 15) && (size_t)(bufEnd - p) >= (size_t)ext + 80;
    const int blk = s * K + r;
    const bool live = live0 && sane;
    if (__ballot(!inside) == 0ull) scan_block<NybWinFast, true>(c, blk, p, ext * 8, ext, cp.pay, bufEnd, live, ringP, ringN);
    else scan_block<NybWin, true>(c, blk, p, ext * 8, ext, cp.pay, bufEnd, live, ringP, ringN);
    if (live0 && !sane) { c.bits[blk] = 0; c.wcScan[blk] = 0; c.draws[blk] = 0; }
    if (live0 && r == 0) {
        // what the synthesis needs to enter the row: whether row 0 holds a block, and the generator state in front of it
        const int pre = (okS && first > 0) ? 1 : 0;
        c.rInfo[s] = make_int2(pre, okS ? (int)cf.row[first - pre].RngState : 0);
        if (okS && !crop) { const int e = first + K - 1; c.packOff[s] = cf.row[e < nI ? e : nI].ByteOffs; }
    }
}


// Block index of packed payloads (ulcx_index_packed_*) - one lane per stream, the walk of k_dscan_packed without its notes:
// per block its start and the state the stream's one generator chain has there (one jump by the block's draws).  It stops
// where k_dscan_packed reports 0 bits.  No stream state, none of the per-block scratch.
// index_walk: one payload (avail bytes at base) into one row of maxBlocks + 1 entries -> the blocks found.
__device__ __forceinline__ int index_walk(const UlcxDecCtx &c, const uint8_t *base, int avail, int maxBlocks, ulcx_index_entry *row) {
    int off = 0, n = 0;
    uint32_t st = 1234567u;                                          // ulcDecoder.c:76
    row[0].ByteOffs = 0; row[0].RngState = st;
    while (n < maxBlocks && off < avail) {
        const Walked w = scan_block<NybWin, false, false>(c, 0, base + off, (avail - off) * 8, avail - off, c.in, c.in + c.inBytes);
        if (!w.bits) break;
        off += (w.bits + 7) >> 3;                                    // the tool rounds every block up to a byte
        st = rng_jump(c.jumpT, st, (uint32_t)w.draws);
        n++;
        row[n].ByteOffs = off; row[n].RngState = st;
    }
    for (int k = n + 1; k <= maxBlocks; k++) { row[k].ByteOffs = -1; row[k].RngState = 0u; }
    return n;
}
__global__ __launch_bounds__(64) void k_dindex(UlcxDecCtx c, int maxBlocks, ulcx_index_entry *index, int32_t *nBlocks) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= c.B) return;
    nBlocks[s] = index_walk(c, c.in + (size_t)s * c.payStride, c.payBytes[s], maxBlocks, index + (size_t)s * ((size_t)maxBlocks + 1));
}
// The same for files that lie back to back (ulcx_index_packed_ragged_*) - one lane per file: file f is bytes [payOffs[f],
// payOffs[f + 1]) of c.in, its row the entries [idxOffs[f], idxOffs[f + 1]) of `index` (idxTotal in all), filled as k_dindex fills
// a row of maxBlocks = capacity - 1.  Payload offsets as corpus_file refuses them, or a row without an entry: a count of 0 and
// nothing written.  (A row of 2^31 entries or more is used up to that: a file below 2^31 bytes has fewer blocks.)  Lanes of one
// wave wait for the longest file among them; the index is built once.
__global__ __launch_bounds__(64) void k_dindex_ragged(UlcxDecCtx c, const int64_t *payOffs, const int64_t *idxOffs, long long idxTotal,
                                                      ulcx_index_entry *index, int32_t *nBlocks) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= c.B) return;
    const long long p0 = payOffs[f], p1 = payOffs[f + 1], i0 = idxOffs[f], i1 = idxOffs[f + 1];
    const bool ok = corpus_bytes_ok(p0, p1, c.inBytes) && i0 >= 0 && i1 > i0 && i1 <= idxTotal;
    if (!ok) { nBlocks[f] = 0; return; }
    const long long cap = i1 - i0 < 0x7FFFFFFFLL ? i1 - i0 : 0x7FFFFFFFLL;
    nBlocks[f] = index_walk(c, c.in + p0, (int)(p1 - p0), (int)cap - 1, index + i0);
}

// Block index of slot-form buffers (ulcx_index_slots_*): the blocks an encode call wrote, each in its own slot with its size
// beside it, so nothing has to be walked in series.  Two launches and no scratch:
//   k_dindex_slots_walk  one lane per (row, block), as k_dscan: the walk of k_dindex, limited to the size the caller gives.  It
//                        parks {the block's bytes, or 0 for a block that is not what its size says; its draws} in the index
//                        entry the block will close (n0 + k + 1: behind the row's entries so far, which nothing touches).
//   k_dindex_slots_scan  one wave per row, 64 blocks per trip: prefix sums of the parked bytes and draws turn each entry into
//                        {byte offset, generator state} - one jump per lane from the trip's start state, which is carried
//                        from trip to trip (a trip's draws stay below 2^30; a row's need not) - and the first block that is
//                        not valid, does not fit the table or would move the offset past an int32 closes the row: it and
//                        everything behind it in the call become {-1, 0}.
// A row whose count is outside [0, indexStride - 1] is skipped by both.  No stream state, none of the per-block scratch.
__global__ __launch_bounds__(256) void k_dindex_begin(long long nEnt, int indexStride, ulcx_index_entry *index, int32_t *nBlocks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nEnt) return;
    const bool head = (i % indexStride) == 0;
    index[i].ByteOffs = head ? 0 : -1; index[i].RngState = head ? 1234567u : 0u;     // ulcDecoder.c:76
    if (head) nBlocks[i / indexStride] = 0;
}
__global__ __launch_bounds__(64) void k_dindex_slots_walk(UlcxDecCtx c, long long nAll, int nBlocks, const int32_t *bits,
                                                          ulcx_index_entry *index, int indexStride, const int32_t *rowBlocks) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    if (id >= nAll) return;
    const long long s = id / nBlocks;
    const int k = (int)(id - s * nBlocks);
    const int n0 = rowBlocks[s];
    if (n0 < 0 || n0 > indexStride - 1 || k >= indexStride - 1 - n0) return;       // no row to append to / no entry left for this block
    const int b = bits[id], nb = b >> 3;
    int bytes = 0, draws = 0;
    if (b > 0 && nb <= c.slot) {
        const int rb = (nb + ((b & 7) ? 1 : 0)) < c.slot ? nb + ((b & 7) ? 1 : 0) : c.slot;
        const Walked w = scan_block<NybWin, false, false>(c, 0, c.in + (size_t)id * c.slot, b, rb, c.in, c.in + c.inBytes);
        if (w.bits > 0 && ((w.bits + 7) >> 3) == nb) { bytes = nb; draws = w.draws; }
    }
    ulcx_index_entry *e = index + (size_t)s * indexStride + n0 + 1 + k;
    e->ByteOffs = bytes; e->RngState = (uint32_t)draws;
}
__global__ __launch_bounds__(64) void k_dindex_slots_scan(const uint32_t *jumpT, int nBlocks, ulcx_index_entry *index, int indexStride, int32_t *rowBlocks) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int n0 = rowBlocks[s];
    if (n0 < 0 || n0 > indexStride - 1) return;
    ulcx_index_entry *row = index + (size_t)s * indexStride;
    const int room = indexStride - 1 - n0, cap = nBlocks < room ? nBlocks : room;   // blocks of the call that have an entry
    long long off = row[n0].ByteOffs;
    uint32_t st = row[n0].RngState;
    int m = 0;
    bool open = true;
    for (int k0 = 0; k0 < cap; k0 += 64) {
        const bool have = k0 + lane < cap;
        ulcx_index_entry *e = row + n0 + 1 + k0 + (have ? lane : 0);
        if (!open) { if (have) { e->ByteOffs = -1; e->RngState = 0u; } continue; }
        int by = 0; uint32_t dr = 0;
        if (have) { by = e->ByteOffs; dr = e->RngState; }
        const bool ok = by > 0;
        if (!ok) { by = 0; dr = 0; }
        // (64 blocks of up to 2^28 bytes: the sum in two halves, each within 32 bits)
        const uint32_t lo = wave_scan_add((uint32_t)by & 0xFFFFu), hi = wave_scan_add((uint32_t)by >> 16);
        const uint32_t dIncl = wave_scan_add(dr);
        const long long end = off + (((long long)hi << 16) + lo);
        const unsigned long long stop = __ballot(have && (!ok || end > 0x7FFFFFFFLL));
        const int here = cap - k0 < 64 ? cap - k0 : 64;
        const int good = stop ? (int)__builtin_ctzll(stop) : here;
        if (have) {
            if (lane < good) { e->ByteOffs = (int)end; e->RngState = rng_jump(jumpT, st, dIncl); }
            else { e->ByteOffs = -1; e->RngState = 0u; }
        }
        m += good;
        if (stop) open = false;
        else {
            off += ((long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 16) + (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
            st = rng_jump(jumpT, st, (uint32_t)__builtin_amdgcn_readlane((int)dIncl, 63));
        }
    }
    if (lane == 0) rowBlocks[s] = n0 + m;
}

// Corpus splice (ulcx_corpus_splice_*): new files from block ranges of resident files.  Output file o is the blocks its
// segments segOffs[o] .. segOffs[o + 1] - 1 name, in order, up to the first one that cannot be taken.  Nothing is walked in
// series, and the output index and segStart are the only working memory; behind k_dindex_begin on the output rows:
//   k_splice_plan  one wave per output file, 64 segments per trip: segStart[j] = the blocks the file's earlier segments plan
//                  (the exclusive sum of max(Count, 0), saturating) - the table the two kernels below search.
//   k_splice_walk  one lane per (output file, output block): the block's segment by binary search, then its source file and
//                  block; the two bounding entries of the source index, and k_dindex_slots_walk's parse of that extent.  It
//                  parks {bytes, draws} in the output entry the block will close; a block that cannot be taken leaves the
//                  {-1, 0} k_dindex_begin wrote there.
//   k_splice_scan  one wave per output file: k_dindex_slots_scan's prefix sums and jumps from an open row, with the byte
//                  capacity as a further stop; the file's bytes, blocks and largest block.
//   k_splice_copy  one lane per aligned 16-byte line of the output payloads: the output block a line begins in by binary search
//                  in the finished row, its source as the walk found it, and on through the blocks the line holds.
// The source corpus and its files are read through corpus_file / file_block, as the indexed walk reads them.
// the segments of output file o: {first, end}, or {0, -1} for a pair that falls or leaves [0, nSeg]
__device__ __forceinline__ int2 splice_segs(const int32_t *segOffs, int o, int nSeg) {
    const int s0 = segOffs[o], s1 = segOffs[o + 1];
    return (s0 >= 0 && s0 <= s1 && s1 <= nSeg) ? make_int2(s0, s1) : make_int2(0, -1);
}
// Output block j of a file with segments [sg.x, sg.y): the source block it names -> {byte offset in its file, bytes} and the
// file in sf; bytes 0 when there is none - j at or behind the plan's end, or a file, a block or index entries that cannot be taken.
// The search: the last segment that starts at or in front of j (zero-count segments in front of it start where it does).
template <bool RAGGED>
__device__ __forceinline__ FileBlock splice_block(const UlcxCorpus &s, const int32_t *segStart, const ulcx_segment *seg, int2 sg, int j, CorpusFile &sf) {
    const FileBlock none = { 0, 0 };
    int lo = sg.x, hi = sg.y;                                       // the last segment that starts at or in front of j
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (segStart[mid] <= j) lo = mid + 1; else hi = mid; }
    if (lo <= sg.x) return none;
    const ulcx_segment g = seg[lo - 1];
    const int r = j - segStart[lo - 1];
    if (r < 0 || r >= g.Count || g.File < 0 || g.File >= s.nFiles || g.First < 0) return none;
    sf = corpus_file(s, (size_t)g.File, RAGGED);
    return file_block(sf, (long long)g.First + r);
}
__global__ __launch_bounds__(64) void k_splice_plan(int nSeg, const int32_t *segOffs, const ulcx_segment *seg, int32_t *segStart) {
    const int o = blockIdx.x, lane = threadIdx.x;
    const int2 sg = splice_segs(segOffs, o, nSeg);
    if (sg.y < 0) {
        // the segments of a bad pair that exist
        const long long a = segOffs[o], b = segOffs[o + 1];
        const int s0 = (int)(a < 0 ? 0 : a > nSeg ? nSeg : a), s1 = (int)(b < 0 ? 0 : b > nSeg ? nSeg : b);
        for (int j = s0 + lane; j < s1; j += 64) segStart[j] = -1;
        return;
    }
    long long carry = 0;
    for (int j0 = sg.x; j0 < sg.y; j0 += 64) {
        const bool have = j0 + lane < sg.y;
        int cnt = have ? seg[j0 + lane].Count : 0;
        cnt = cnt < 0 ? 0 : cnt;
        // (64 counts of up to 2^31 - 1: the sum in two halves, each within 32 bits)
        const uint32_t lo = wave_scan_add((uint32_t)cnt & 0xFFFFu), hi = wave_scan_add((uint32_t)cnt >> 16);
        const long long incl = carry + (((long long)hi << 16) + lo), excl = incl - cnt;
        if (have) segStart[j0 + lane] = excl > 0x7FFFFFFFLL ? 0x7FFFFFFF : (int)excl;
        carry += ((long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 16) + (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
    }
}
template <bool RAGGED>
__global__ __launch_bounds__(64) void k_splice_walk(UlcxDecCtx c, UlcxCorpus s, long long nAll, int nSeg, const int32_t *segOffs, const ulcx_segment *seg,
                                                    const int32_t *segStart, ulcx_index_entry *outIndex, int outIndexStride) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    if (id >= nAll) return;
    const int per = outIndexStride - 1;
    const long long o = id / per;
    const int j = (int)(id - o * per);
    const int2 sg = splice_segs(segOffs, (int)o, nSeg);
    CorpusFile sf;
    const FileBlock b = splice_block<RAGGED>(s, segStart, seg, sg, j, sf);
    if (!b.ext) return;
    const Walked w = scan_block<NybWin, false, false>(c, 0, sf.base + b.off, b.ext * 8, b.ext, c.in, c.in + c.inBytes);
    if (w.bits <= 0 || ((w.bits + 7) >> 3) != b.ext) return;
    ulcx_index_entry *e = outIndex + (size_t)o * outIndexStride + 1 + j;
    e->ByteOffs = b.ext; e->RngState = (uint32_t)w.draws;
}
__global__ __launch_bounds__(64) void k_splice_scan(const uint32_t *jumpT, ulcx_index_entry *outIndex, int outIndexStride, long long outPayStride,
                                                    int32_t *outPayBytes, int32_t *outMaxBlock, int32_t *outBlocks) {
    const int o = blockIdx.x, lane = threadIdx.x;
    ulcx_index_entry *row = outIndex + (size_t)o * outIndexStride;
    const int cap = outIndexStride - 1;
    const long long room = outPayStride < 0x7FFFFFFFLL ? outPayStride : 0x7FFFFFFFLL;
    long long off = 0;
    uint32_t st = 1234567u;                                          // ulcDecoder.c:76
    int m = 0;
    uint32_t mx = 0;
    bool open = true;
    for (int k0 = 0; k0 < cap; k0 += 64) {
        const bool have = k0 + lane < cap;
        ulcx_index_entry *e = row + 1 + k0 + (have ? lane : 0);
        if (!open) { if (have) { e->ByteOffs = -1; e->RngState = 0u; } continue; }
        int by = 0; uint32_t dr = 0;
        if (have) { by = e->ByteOffs; dr = e->RngState; }
        const bool ok = by > 0;
        if (!ok) { by = 0; dr = 0; }
        const uint32_t lo = wave_scan_add((uint32_t)by & 0xFFFFu), hi = wave_scan_add((uint32_t)by >> 16);
        const uint32_t dIncl = wave_scan_add(dr);
        const long long end = off + (((long long)hi << 16) + lo);
        const unsigned long long stop = __ballot(have && (!ok || end > room));
        const int here = cap - k0 < 64 ? cap - k0 : 64;
        const int good = stop ? (int)__builtin_ctzll(stop) : here;
        if (have) {
            if (lane < good) { e->ByteOffs = (int)end; e->RngState = rng_jump(jumpT, st, dIncl); }
            else { e->ByteOffs = -1; e->RngState = 0u; }
        }
        mx = umax32(mx, (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max(lane < good ? (uint32_t)by : 0u), 63));
        m += good;
        if (stop) {
            open = false;
            if (good > 0) off += ((long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, good - 1) << 16) + (uint32_t)__builtin_amdgcn_readlane((int)lo, good - 1);
        } else {
            off += ((long long)(uint32_t)__builtin_amdgcn_readlane((int)hi, 63) << 16) + (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
            st = rng_jump(jumpT, st, (uint32_t)__builtin_amdgcn_readlane((int)dIncl, 63));
        }
    }
    if (lane == 0) { outBlocks[o] = m; outPayBytes[o] = (int)off; if (outMaxBlock) outMaxBlock[o] = (int)mx; }
}
// 16 bytes from any address: the aligned words that hold them (4, or 5 for a source off its words), put together by shifts
__device__ __forceinline__ uint4 splice_load16(const uint8_t *src) {
    const unsigned sh = (unsigned)((uintptr_t)src & 3u) * 8u;
    const uint32_t *sw = (const uint32_t *)(src - (sh >> 3));
    uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2], w3 = sw[3];
    if (sh) {
        const uint32_t w4 = sw[4];
        w0 = (w0 >> sh) | (w1 << (32u - sh)); w1 = (w1 >> sh) | (w2 << (32u - sh));
        w2 = (w2 >> sh) | (w3 << (32u - sh)); w3 = (w3 >> sh) | (w4 << (32u - sh));
    }
    return make_uint4(w0, w1, w2, w3);
}
#define SPLICE_COPY_WG 256
template <bool RAGGED>
__global__ __launch_bounds__(SPLICE_COPY_WG) void k_splice_copy(UlcxCorpus s, long long nAll, long long lines, int nSeg, const int32_t *segOffs, const ulcx_segment *seg,
                                                                const int32_t *segStart, const ulcx_index_entry *outIndex, int outIndexStride,
                                                                const int32_t *outBlocks, uint8_t *outPay, long long outPayStride) {
    const long long id = (long long)blockIdx.x * SPLICE_COPY_WG + threadIdx.x;
    if (id >= nAll) return;
    const long long o = id / lines, line = id - o * lines;
    const int nB = outBlocks[o];
    if (nB <= 0) return;
    const ulcx_index_entry *row = outIndex + (size_t)o * outIndexStride;
    const int total = row[nB].ByteOffs;
    uint8_t *dst = outPay + (size_t)o * (size_t)outPayStride;
    // the line: bytes [a, z) of the file, z - a == 16 everywhere but at the file's two ends
    const long long l0 = line * 16 - (long long)((uintptr_t)dst & 15u);
    const int a = l0 < 0 ? 0 : (int)(l0 < total ? l0 : total), z = l0 + 16 < total ? (int)(l0 + 16) : total;
    if (a >= z) return;
    int lo = 0, hi = nB;                                             // the block byte a lies in: the last one that starts at or in front of it
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (row[mid].ByteOffs <= a) lo = mid + 1; else hi = mid; }
    int blk = lo - 1;
    const int2 sg = splice_segs(segOffs, (int)o, nSeg);
    uint32_t v[4] = { 0u, 0u, 0u, 0u };
    bool whole = false;
    for (int at = a; at < z; blk++) {
        const int b0 = row[blk].ByteOffs, b1 = row[blk + 1].ByteOffs, end = b1 < z ? b1 : z;
        CorpusFile sf;
        const FileBlock b = splice_block<RAGGED>(s, segStart, seg, sg, blk, sf);
        if (b.ext != b1 - b0) return;                               // (not what the walk saw: tables that changed under the call)
        const uint8_t *src = sf.base + b.off + (at - b0);
        if (end - at == 16) { const uint4 x = splice_load16(src); v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; whole = true; }
        else for (int i = at; i < end; i++) {
            const unsigned q = (unsigned)(i - a), x = (unsigned)src[i - at] << ((q & 3u) * 8u);
            v[0] |= (q >> 2) == 0u ? x : 0u; v[1] |= (q >> 2) == 1u ? x : 0u; v[2] |= (q >> 2) == 2u ? x : 0u; v[3] |= (q >> 2) == 3u ? x : 0u;
        }
        at = end;
    }
    if (whole || z - a == 16) *(uint4 *)(dst + a) = make_uint4(v[0], v[1], v[2], v[3]);
    else for (int i = 0; i < z - a; i++) dst[a + i] = (uint8_t)((i < 4 ? v[0] : i < 8 ? v[1] : i < 12 ? v[2] : v[3]) >> ((i & 3) * 8));
}

#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// float index inside a padded FFT array (two floats of padding after every 32): complex n sits at FFT_PADS(n, DPS)
__device__ __forceinline__ int padf(int f) { return f + ((f >> (DPS + 1)) << 1); }      // float index into a padded array of complex

// Noise runs found while decoding a unit, 8 bytes each:
//   x = first coefficient | count << 16 (count - 1 for a tail, which may span the whole unit) | tail << 31
//   y = draws made in the unit before the run | level << 16 | quantizer index << 21
#ifdef ULCX_DSYN_STAMPS
#define DSYN_NSTAMP 20
struct DsynStamps { unsigned long long t[DSYN_NSTAMP], t0; };
#define SWAITALL() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")      // diagnostic: the stamp behind it sees the wait for everything in flight
#define SSTAMP(sw, i) do { if ((sw).stp) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); (sw).stp->t[i] += t_ - (sw).stp->t0; (sw).stp->t0 = t_; } } while (0)
#else
#define SSTAMP(sw, i) do {} while (0)
#define SWAITALL() do {} while (0)
#endif
struct SynWave {                 // one wave's working set while it synthesises one (channel, subblock) unit
    float *A;                    // the unit's coefficients = the FFT's input array (LDS, padded)
    int   *pre;                  // 64 prefix counts (LDS)
    uint32_t *seedTab;           // the unit's sign-parity stream P (LDS, synth_noise)
    int lane;
#ifdef ULCX_DSYN_STAMPS
    DsynStamps *stp;
#endif
};
#define SEEDTAB_DRAWS 2048       // draws of a unit the table covers; pieces beyond it jump on their own

// Noise synthesis (ulcDecoder.c:146-160, :166-186).  The decoder draws one xorshift value per noise coefficient and
// only ever looks at its top bit: the sign of the run's level flips, cumulatively, on every draw with the top bit set.
//   1. the unit's draws, densely: lane l owns draws 32l+1 .. 32l+32; its word of P (bit n of the stream = parity of the top
//      bits of draws 1 .. n+1) is the parity prefix of those 32 top bits - a linear function of the unit's start state, read
//      from tables (par_word) - completed by a parity carry across the lanes.  P goes to LDS (2048 bits per pass).
//   2. one lane per (run, 32-coefficient chunk) piece: 32 sign bits are a window of P (xor the parity at the run's
//      start), the level is the run's constant or the tail's chain value at the chunk (k_dscan) decaying from there.
// No sequential generator in step 2, no jumps, and every coefficient is written exactly once.
// A lane's word of a unit's sign-parity stream P, from the state the (pass of the) unit starts from: bit i = parity of the top
// bits of draws 32 lane + 1 .. 32 lane + i + 1.  Linear in the state: four byte tables per lane (host: build_rng_tables), and
// since the state is the same in all lanes, each look-up is ONE coalesced row of 64 words (c.parT [4][256][lane]).
__device__ __forceinline__ uint32_t par_word(const uint32_t *__restrict__ parT, uint32_t st, int lane) {
    const uint32_t *J = parT + lane;
    return J[(st & 255u) << 6] ^ J[(256u + ((st >> 8) & 255u)) << 6] ^ J[(512u + ((st >> 16) & 255u)) << 6] ^ J[(768u + (st >> 24)) << 6];
}
// LOW (the low-rate source mode, SynLow): only the pieces below coefficient `keep` are written - keep is a multiple of 32, so a
// piece lies on one side of it -, while P still covers every draw of the unit: a kept coefficient's draw index counts them all.
template <bool LOW = false>
__device__ __forceinline__ void synth_noise(const UlcxDecCtx &c, const SynWave &sw, const uint2 *__restrict__ list, int nE, const uint2 ent0, uint32_t x0, uint32_t unitSeed, int unitDraws,
                                            float tailRR, const float *tailMag, int keep = 0) {
    const int lane = sw.lane;
    uint32_t *P = sw.seedTab;                                 // the unit's whole stream: max(64, BS/32) words + a zero word
    // (ent0: round 0 of the run list, x0: the lane's word of the first pass - both fetched by the caller with the unit's first records)
    // ---- 1. sign-parity stream, 2048 draws per pass (one pass unless the unit has more than 2048 noise coefficients)
    uint32_t passPar = 0;                                     // parity of the top bits of all earlier passes
    for (int dbase = 0; dbase < unitDraws; dbase += 2048) {
        // bit i of x = parity of the top bits of draws dbase+32*lane+1 .. +i+1 (bit 31: of all 32)
        const uint32_t x = (dbase == 0) ? x0 : par_word(c.parT, rng_jump(c.jumpT, unitSeed, (uint32_t)dbase), lane);
        const unsigned long long odd = __ballot((int)x < 0);
        const uint32_t carry = ((uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(odd >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)odd, 0)) + passPar) & 1u;
        P[(dbase >> 5) + lane] = carry ? ~x : x;
        passPar ^= (uint32_t)__popcll(odd) & 1u;
    }
    if (lane == 0) P[((unitDraws + 2047) >> 11) << 6] = 0u;   // the word behind the last pass: windows at the very end read it
    WAVE_SYNC();
    {
        // ---- 2. pieces
        for (int e0 = 0; e0 < nE; e0 += 64) {
            const int e = e0 + lane;
            const bool have = e < nE;
            const uint2 ent = (e0 == 0) ? ent0 : (have ? list[e] : make_uint2(0u, 0u));
            const int pos = ent.x & 0xFFFF, isTail = (int)(ent.x >> 31);
            const int np = (int)((ent.x >> 16) & 0x7FFF) + isTail;
            int nseg = have ? ((pos + np - 1) >> 5) - (pos >> 5) + 1 : 0;
            if constexpr (LOW) {                                    // the run's pieces below `keep` (a run at or behind it: none)
                const int lastC = (pos + np - 1) >> 5, keepC = (keep >> 5) - 1;
                nseg = (have && pos < keep) ? (lastC < keepC ? lastC : keepC) - (pos >> 5) + 1 : 0;
            }
            const uint32_t incl = wave_scan_add((uint32_t)nseg);
            const int total = __builtin_amdgcn_readlane((int)incl, 63);
            sw.pre[lane] = have ? (int)(incl - nseg) : 0x7FFFFFFF;
            WAVE_SYNC();
            for (int sb = 0; sb < total; sb += 64) {
                const int si = sb + lane;
                const bool act = si < total;
                // the run this piece belongs to: the last one whose first piece is at or before si
                int lo = 0, hi = 63;
#pragma unroll
                for (int it = 0; it < 6; it++) { int mid = (lo + hi + 1) >> 1; bool le = sw.pre[mid] <= si; lo = le ? mid : lo; hi = le ? hi : mid - 1; }
                const int j = act ? lo : 0;
                const uint32_t ex = (uint32_t)__builtin_amdgcn_ds_bpermute(j << 2, (int)ent.x);
                const uint32_t ey = (uint32_t)__builtin_amdgcn_ds_bpermute(j << 2, (int)ent.y);
                const int first = __builtin_amdgcn_ds_bpermute(j << 2, (int)(incl - nseg));
                const int rpos = ex & 0xFFFF, rtail = (int)(ex >> 31), rnp = (int)((ex >> 16) & 0x7FFF) + rtail;
                const int d0 = ey & 0xFFFF, lvl = (ey >> 16) & 31, qi = (ey >> 21) & 63;
                const int chunk = (rpos >> 5) + (act ? si - first : 0);          // (idle lanes shadow the first piece of run 0: every address they form is valid)
                const int plo = rpos > (chunk << 5) ? rpos : (chunk << 5);
                const int phi = (rpos + rnp) < ((chunk << 5) + 32) ? (rpos + rnp) : ((chunk << 5) + 32);
                const int off = plo - rpos;
                const int dc = d0 + off;                                         // draws of the unit in front of the piece's first coefficient
                const int n = act ? phi - plo : 0;
                // sign bits of the piece: P bits dc .. dc+31 (parity after its i-th draw), relative to the parity where the run began
                uint32_t win = __builtin_amdgcn_alignbit(P[(dc >> 5) + 1], P[dc >> 5], dc & 31);
                uint32_t s0 = 0;                                                 // parity where the run began
                if (d0 > 0) s0 = (P[(d0 - 1) >> 5] >> ((d0 - 1) & 31)) & 1u;
                win ^= 0u - s0;
                const float quant = expand_quantizer(qi);
                float mag = (float)(lvl * lvl) * quant * (rtail ? (1.0f / 16) : (1.0f / 4));      // ulcDecoder.c:146-150, :166-170
                if (rtail && off > 0) mag = tailMag[chunk];                                         // the tail's chain at coefficient 32*chunk (k_dscan)
                const float rr = rtail ? tailRR : 1.0f;
                float *dst = sw.A + padf(plo);                                                      // (DPS 4: a piece never crosses a padding gap; DPS 3: up to two)
                constexpr int GAPF = 2 << DPS;                                                      // floats between two padding gaps
                const int g1 = GAPF - (plo & (GAPF - 1));                                           // piece elements in front of the first gap
                SSTAMP(sw, 9);
#pragma unroll
                for (int i = 0; i < 32; i++) {
                    // ulcDecoder.c:156-160 / :181-184: flip on the draw's top bit (cumulative), store, decay (r = 1 for runs)
                    const float v = __uint_as_float(__float_as_uint(mag) | ((win << (31 - i)) & 0x80000000u));
                    if (i < n) dst[GAPF >= 32 ? i : i + (i >= g1 ? 2 : 0) + (i >= g1 + GAPF ? 2 : 0)] = v;
                    mag *= rr;
                }
            }
            WAVE_SYNC();
        }
    }
}

// Dequantise one (channel, subblock) unit into A[0 .. S) (zeroed by the caller) from what the scan left: one lane per
// plain-run record (up to seven coefficients each, ulcDecoder.c:69-73), then the noise runs (synth_noise).
// ur = {first plain-run record, their count, first noise record, their count} of the unit.
// LOW: S is the leading part of the unit that is kept (its reduced size); the records and the draws are the full unit's.
template <bool LOW = false>
__device__ __forceinline__ void synth_unit(const UlcxDecCtx &c, const SynWave &sw, int S, const uint2 *__restrict__ prec, const uint2 *__restrict__ nrec,
                                           int4 ur, uint32_t unitSeed, int unitDraws, float tailRR, const float *tailMag, int zeroFloat2 = 0) {
    const int lane = sw.lane;
    // the lane's word of the unit's sign-parity stream (synth_noise): four coalesced table rows from the unit's start state, in
    // flight behind the zero fill and the scatter (round 5; a two-step jump to the lane's own state - eight 64-address gathers -
    // and 32 draws before: the noise synthesis waited 2-3 k cycles for them)
    const uint32_t x0 = par_word(c.parT, unitSeed, lane);
    const uint2 *pr = prec + ur.x;
    // rounds 0..2 of the plain-run records: in flight behind the zero fill (one round trip to memory, not one per round)
    const uint2 recFirst = (lane < ur.y) ? pr[lane] : make_uint2(0u, 0u);
    const uint2 rec1 = (lane + 64 < ur.y) ? pr[lane + 64] : make_uint2(0u, 0u), rec2 = (lane + 128 < ur.y) ? pr[lane + 128] : make_uint2(0u, 0u);
    const uint2 ent0 = (lane < ur.w) ? nrec[ur.z + lane] : make_uint2(0u, 0u);       // round 0 of the noise runs: one round trip for all of the unit's lists
    if (zeroFloat2) {                                            // (the caller's array: cleared here, behind the loads above)
        float2 *Az = (float2 *)sw.A;
        for (int i = lane; i < zeroFloat2; i += 64) Az[i] = make_float2(0.0f, 0.0f);
        WAVE_SYNC();
    }
    SSTAMP(sw, 12);
    SWAITALL();
    SSTAMP(sw, 13);
    for (int r0 = 0; r0 < ur.y; r0 += 64) {
        const int r = r0 + lane;
        if (r < ur.y) {
            const uint2 rec = (r0 == 0) ? recFirst : (r0 == 64) ? rec1 : (r0 == 128) ? rec2 : pr[r];
            const int pos = rec.x & 0x7FFF, qi = (rec.x >> 15) & 31, m = (rec.x >> 20) & 7;
            const float quant = expand_quantizer(qi);
            float *dst = sw.A + padf(pos);
            const int gap = (2 << DPS) - (pos & ((2 << DPS) - 1));   // coefficients before the next padding gap (a run of <= 7 crosses at most one)
#pragma unroll
            for (int i = 0; i < 7; i++) {
                int sv = (int)((rec.y >> (4 * i)) & 0xF);
                sv = (sv ^ 0x8) - 0x8;
                sv = (sv < 0) ? (-sv * sv) : (+sv * sv);
                if (i < m && pos + i < S) dst[i + (i >= gap ? 2 : 0)] = (float)sv * quant;
            }
        }
    }
    SSTAMP(sw, 8);
    if (ur.w > 0) {
        if constexpr (LOW) synth_noise<true>(c, sw, nrec + ur.z, ur.w, ent0, x0, unitSeed, unitDraws, tailRR, tailMag, S);
        else synth_noise(c, sw, nrec + ur.z, ur.w, ent0, x0, unitSeed, unitDraws, tailRR, tailMag);
    }
    SSTAMP(sw, 10);
    WAVE_SYNC();
}

// ---------------------------------------------------------------------------
// Time domain of one channel of a DECIMATED block of a stereo stream, by one wave (ulcDecoder.c:219-273).
// The reference keeps BS/2 pending samples per channel in TransformInvLap, time-reversed: the tail of the last subblock
// (to be overlapped with the next) in front, behind it a FIFO that delays decimated subblocks to the centre of the
// block, and it moves the FIFO once per subblock.  Read in time order (P[n] = Lap[BS/2-1-n]) the two parts are ONE list,
// and a subblock of size S at coefficient offset off only ever (i) replaces the M = S/2 pending samples in front of
// time off by the first half of its windowed output, (ii) appends the second half and (iii) appends its own tail:
//     T[off-M+p]     = c A - s B      A = T[off-M+p], B = z[M+p]          (pass-through below the ramp)
//     T[off+M-1-p]   = s A + c B
//     T[off+M+i]     = z[M-1-i]
// on the timeline T = [pending (times -BS/2..-1) | this block's BS new samples]; the block's output is T[-BS/2 .. BS/2)
// and T[BS/2 .. BS) is the new pending list.  Nothing is shifted.  T's non-negative times live in the channel's FFT
// array (a subblock's spectrum sits at [off, off+S): everything it writes at times >= off lands in its own region, so
// "all lanes read, wave barrier, all lanes write" is enough), negative times in the lapping state L (L[-1-t]).
// Returns the size of the last subblock; the caller emits the output and stores the new pending list (dec_time_finish).
// DEC_MAXT = (BlockSize/2)/64 register slots per lane: a template parameter of the kernel (16: BlockSize <= 2048, 32: <= 4096)
// ---------------------------------------------------------------------------
template <int DEC_MAXT>
__device__ __forceinline__ int dec_time_wave(const UlcxDecCtx &c, float2 *zc, float *L, int wc, unsigned pat0, int nsub, int lastSub, int lane) {
    const int BS = c.BS;
    float *arr = (float *)zc;                                    // times >= 0, padded
    int last = lastSub;
    unsigned pat = pat0; int off = 0;
    for (int j = 0; j < nsub; j++, pat >>= 4) {
        const int d = pat & 7, S = BS >> d, M = S >> 1;
        int ov = S;                                              // ulcDecoder.c:234-239
        if (pat & 8) ov >>= (wc & 7);
        if (ov > last) ov = last;
        last = S;
        const float2 *zj = zc + FFT_PADS(off >> 1, DPS);
        const float2 *pre = c.T.pre[d];
        const int a = (S - ov) >> 1;
        const float *fall = c.T.winFall + ov, *rise = c.T.winRise + ov;
        const int bits = 31 - __clz(M);
        const int tA = off - M;                                  // time of A(0)
        // post-twiddle fused with the windowed overlap (oracle/orc_fourier.c orc_imdct): pair p: A = T[tA+p], B = z[M+p]
        float o[DEC_MAXT / 4][4], nl[DEC_MAXT / 4][2];
#pragma unroll
        for (int t = 0; t < DEC_MAXT / 4; t++) {
            const int kk = lane + 64 * t;
            if (kk < M / 2) {
                const int k1 = kk, k2 = M - 1 - kk;
                const int r1 = FFT_PADS((int)(__brev((unsigned)k1) >> (32 - bits)), DPS);
                const int r2 = FFT_PADS((int)(__brev((unsigned)k2) >> (32 - bits)), DPS);
                const float2 y1 = cmulc_post(zj[r1], pre[k1]), y2 = cmulc_post(zj[r2], pre[k2]);     // (Re y, -Im y)
                const int   pv[2] = { M - 1 - 2 * k1, M - 2 - 2 * k1 };
                float Av[2];
                // (L may be global memory, arr is LDS: separate branches, never a select between the two pointers)
                if (tA + pv[1] < 0) { Av[0] = L[-1 - (tA + pv[0])]; Av[1] = L[-1 - (tA + pv[1])]; }      // (pv[1] = pv[0]-1, even time: both on the same side of 0)
                else { Av[0] = arr[padf(tA + pv[0])]; Av[1] = arr[padf(tA + pv[1])]; }
                const float Bv[2] = { y1.y, y2.x };
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int p = pv[q];
                    const float A = Av[q], B = Bv[q];
                    if (p < a) { o[t][2 * q] = A; o[t][2 * q + 1] = B; }
                    else {
                        const float cw = fall[p - a], sn = rise[p - a];
                        const float m1 = sn * B, m3 = cw * B;               // spec v2: fused (orc_imdct)
                        o[t][2 * q] = __builtin_fmaf(cw, A, -m1);
                        o[t][2 * q + 1] = __builtin_fmaf(sn, A, m3);
                    }
                }
                nl[t][0] = y1.x; nl[t][1] = y2.y;               // z[2 k1], z[2 k1 + 1]: the tail at times off+M+pv[0], off+M+pv[1]
            }
        }
        WAVE_SYNC();
#pragma unroll
        for (int t = 0; t < DEC_MAXT / 4; t++) {
            const int kk = lane + 64 * t;
            if (kk < M / 2) {
                const int p0 = M - 1 - 2 * kk, p1 = p0 - 1;
                if (tA + p1 < 0) { L[-1 - (tA + p0)] = o[t][0]; L[-1 - (tA + p1)] = o[t][2]; }
                else { arr[padf(tA + p0)] = o[t][0]; arr[padf(tA + p1)] = o[t][2]; }
                arr[padf(off + M - 1 - p0)] = o[t][1]; arr[padf(off + M - 1 - p1)] = o[t][3];
                arr[padf(off + M + p0)] = nl[t][0]; arr[padf(off + M + p1)] = nl[t][1];
            }
        }
        WAVE_SYNC();
        off += S;
    }
    return last;
}

// ---------------------------------------------------------------------------
// Output samples.  OUT = float: the C API's layout; OUT = int16_t: PCM16 output, converted on store
// exactly as the reference's WAV writer does (tools/WavIO_Helper.c:9-13,56-63: lrintf(clamp(x * 2^15, -32768, 32767))).
// (the decoded samples are written once and not read again by the decoder: non-temporal)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st1(float *p, float a) { __builtin_nontemporal_store(a, p); }
__device__ __forceinline__ void st2(float *p, float a, float b) { f32x2 w = { a, b }; __builtin_nontemporal_store(w, (f32x2 *)p); }
__device__ __forceinline__ void st4(float *p, float a, float b, float d, float e) { f32x4 w = { a, b, d, e }; __builtin_nontemporal_store(w, (f32x4 *)p); }
__device__ __forceinline__ void st1(int16_t *p, float a) { *p = to_pcm16(a); }
__device__ __forceinline__ void st2(int16_t *p, float a, float b) { *(short2 *)p = make_short2(to_pcm16(a), to_pcm16(b)); }
__device__ __forceinline__ void st4(int16_t *p, float a, float b, float d, float e) { *(short4 *)p = make_short4(to_pcm16(a), to_pcm16(b), to_pcm16(d), to_pcm16(e)); }
template <typename OUT> __device__ __forceinline__ OUT *out_base(const UlcxDecCtx &c);
template <> __device__ __forceinline__ float *out_base<float>(const UlcxDecCtx &c) { return c.pcm; }
template <> __device__ __forceinline__ int16_t *out_base<int16_t>(const UlcxDecCtx &c) { return c.pcm16; }

// ---------------------------------------------------------------------------
// Sample-crop store mode (ulcx_decode_crops_samples_*): a row of the call is nSamples samples from sample `skip` of its first
// block on, and the output is channels-first, [row][channel][nSamples].  The synthesis is the range synthesis, block for block;
// only where a sample goes changes: sample m of output block kOut of a row belongs at t = kOut * BlockSize + m - skip of each
// channel's plane, it is stored when t lies in [0, nSamples), and as 0 when t >= len (the row's length).  Both kernels take the
// mode's fields in their one further argument (SynSamples, below): no other instantiation sees any of it.
// One (row, block)'s clip is three bounds on m and is the same for every thread: scalars.
struct UlcxSampArg { const int32_t *skip, *len; int nSamples; };      // [rows] each, written by k_crop_sample_rows
template <typename OUT>
struct SampBlk {
    OUT *org;                    // where sample m = 0 of channel 0 would go (in front of the plane when the row starts inside the block: an address only)
    int nS;                      // elements per plane
    int mLo, mHi, mLen;          // m in [mLo, mHi) is stored; m >= mLen as 0
    __device__ __forceinline__ OUT *plane(int ch) const { return org + (long long)ch * nS; }
    // a sample pair at an even m of this plane may go out as one store
    static __device__ __forceinline__ bool pairs(const OUT *pl) { return ((uintptr_t)pl & (2 * sizeof(OUT) - 1)) == 0; }
    // (m is never negative and a block is below 2^32 bytes: a uniform base and a 32-bit byte offset per thread)
    static __device__ __forceinline__ OUT *at(OUT *pl, int m) { return (OUT *)((char *)pl + (unsigned)m * (unsigned)sizeof(OUT)); }
    __device__ __forceinline__ void one(OUT *pl, int m, float v) const {
        if (m >= mLo && m < mHi) st1(at(pl, m), m < mLen ? v : 0.0f);
    }
    // samples m (even) and m + 1; al = pairs(pl)
    __device__ __forceinline__ void two(OUT *pl, bool al, int m, float v0, float v1) const {
        if (al && m >= mLo && m + 1 < mHi) st2(at(pl, m), m < mLen ? v0 : 0.0f, m + 1 < mLen ? v1 : 0.0f);
        else { one(pl, m, v0); one(pl, m + 1, v1); }
    }
    // a dead block: zeros wherever the block has samples of the row
    __device__ __forceinline__ void zero(int C, int tid) const {
        for (int ch = 0; ch < C; ch++) { OUT *pl = plane(ch); for (int m = mLo + tid; m < mHi; m += WG) st1(at(pl, m), 0.0f); }
    }
};
template <typename OUT>
__device__ __forceinline__ SampBlk<OUT> samp_blk(OUT *base, int C, int BS, int nS, int row, int kOut, int skip, int len) {
    SampBlk<OUT> b;
    const long long lo = (long long)skip - (long long)kOut * BS;      // m of the row's sample 0
    b.nS = nS;
    b.org = base + ((long long)row * C * nS - lo);
    b.mLo = lo > 0 ? (int)lo : 0;
    b.mHi = lo + nS < BS ? (int)(lo + nS) : BS;                        // (a block behind the row's samples: mHi <= mLo, nothing stored)
    b.mLen = lo + len < BS ? (int)(lo + len) : BS;
    return b;
}
// The rows of a sample-crop call, one lane per row: (start, len) -> the block range the crop walk works on and what the stores
// clip by.  first = start / BlockSize, skip = start % BlockSize, count = the blocks samples [skip, skip + len) touch, len clamped
// to [0, nSamples] (NULL: nSamples).  A start the walk must refuse - negative, or a block number no index can hold - becomes
// first = -1: the row comes back as zeros, as a crop row with that first does.
__global__ __launch_bounds__(64) void k_crop_sample_rows(int n, int BS, int nSamples, const int64_t *start, const int32_t *len,
                                                         int32_t *first, int32_t *count, int32_t *skip, int32_t *lenC) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const long long st = start[i];
    int l = len ? len[i] : nSamples;
    l = l < 0 ? 0 : l > nSamples ? nSamples : l;
    const long long b = st / BS;
    const bool ok = st >= 0 && b < 0x40000000LL;
    const int sk = ok ? (int)(st - b * BS) : 0;
    first[i] = ok ? (int)b : -1;
    count[i] = (ok && l > 0) ? (int)(((long long)sk + l - 1) / BS) + 1 : 0;
    skip[i] = sk;
    lenC[i] = ok ? l : 0;
}

// ---------------------------------------------------------------------------
// Plane source mode (ulcx_synth_spectra_*): the synthesis of caller-held coefficients.  SynPlanes<LR>, a range launch in the sample
// store mode: where the other instantiations dequantise a unit from the walk's records (synth_unit), these load its S floats from the row's plane - coef
// [row][channel][nPl][BS], a block's subblocks in coded order, what the spectra calls write - into the same padded array, and
// everything behind that is the one shared text.  No walk has run: k_synth_rows wrote the rows the synthesis reads (window
// codes, liveness), and nothing of the walk's records, draws or generator states is looked at.
// LR: the planes hold left/right already - the time-domain un-mix (ulcDecoder.c:281-289) is skipped, each channel stored as it stands.
// Row k of a stream's K per-block rows is plane k - (K - nPl): nPl = K when plane 0 is the block in front (ULCX_SYNTH_WARM), else K - 1.
// Low-rate source mode (ulcx_decode_crops_lowrate_*): SynLow, a range launch in the sample store mode.  The walk has run at the
// file's BlockSize BSw; the context this synthesis gets is that of BlockSize BS = BSw >> lgD - geometry, tables, lapping rows -
// while the per-block rows, the records and their strides are still the walk's.  A unit of S coefficients is dequantised up to
// its leading S >> lgD (synth_unit<true>: the records and the draws are the full unit's) and everything behind that is the one
// shared text at BS: the reference decoder of BlockSize BS whose TransformBuffer holds the low bins.  The per-wave lists (the
// sign-parity stream covers the FULL unit's draws) are sized by BSw.
// words of a wave's sign-parity stream: by the BlockSize of the walk
#define DSYN_PWORDS(BS) (((BS) / 32 > 64 ? (BS) / 32 : 64) + 2)
// Synthesis modes: what kind of call a launch of k_dsyn / k_dgen serves, one type per kind (host side: UlcxSynKind).  The mode is the
// kernel's template parameter MODE and its one further argument: constants that say what the kernel text compiles in, and the
// fields only that kind of call has.
//   split  the grid is an even cut of the (stream, block) pairs (k_dsyn; k_dgen ignores it)
//   range  streams are entered from nothing, through the block in front (a range call, and everything built on one)
//   samp   the sample store mode: s, the rows' clips
//   plane  the plane source mode (no records, no generator): unit(), where a unit's coefficients lie;  lr: the planes hold left/right
//   low    the low-rate source mode (the records clipped to the reduced units): pwords(), the sign-parity words of the walk's BlockSize
//   part   one coded channel per pair (ulcx_decode_crops_part_*, SynPart): the low-rate source mode over the coded channels part, part + 2, ...
//          alone, each stored as it stands - no un-mix - into plane ch >> 1 of nOut (k_dgen, or k_dpart for stereo: syn_pick; never k_dsyn)
#define SYN_MODE(SPLIT, RANGE, SAMP, PLANE, LR_, LOW) static constexpr bool split = SPLIT, range = RANGE, samp = SAMP, plane = PLANE, lr = LR_, low = LOW, part = false
struct SynWhole   { SYN_MODE(false, false, false, false, false, false); };       // one workgroup per stream, from and to the stream's state
struct SynCut     { SYN_MODE(true,  false, false, false, false, false); };       // the same call over a cut
struct SynRange   { SYN_MODE(true,  true,  false, false, false, false); };       // range and crop calls
struct SynSamples { SYN_MODE(true,  true,  true,  false, false, false); UlcxSampArg s; };
template <bool LR_> struct SynPlanes {
    SYN_MODE(true, true, true, true, LR_, false); UlcxSampArg s; const float *coef; int nPl;
    __device__ __forceinline__ const float *unit(int row, int C, int ch, int K, int k, int BS) const { return coef + (((size_t)row * C + ch) * nPl + (k - (K - nPl))) * (size_t)BS; }
};
struct SynLow { SYN_MODE(true, true, true, false, false, true); UlcxSampArg s; int BSw; __device__ __forceinline__ int pwords() const { return DSYN_PWORDS(BSw); } };
#undef SYN_MODE
struct SynPart : SynLow { static constexpr bool part = true; int which, nOut; };   // which: ULCX_PART_MID / ULCX_PART_SIDE; nOut: the planes of a row
template <typename MODE> __device__ __forceinline__ int syn_pwords(const MODE &m, int BS) { if constexpr (MODE::low) return m.pwords(); else return DSYN_PWORDS(BS); }
// a range call enters streams as a cut does; sample crops are range launches; both sources store samples
template <typename M> constexpr bool syn_mode_ok = (!M::range || M::split) && (!M::samp || M::range) && (!M::plane || M::samp) && (!M::lr || M::plane) && (!M::low || (M::samp && !M::plane));
static_assert(syn_mode_ok<SynWhole> && syn_mode_ok<SynCut> && syn_mode_ok<SynRange> && syn_mode_ok<SynSamples> && syn_mode_ok<SynPlanes<false>> && syn_mode_ok<SynPlanes<true>> && syn_mode_ok<SynLow>);
static_assert(syn_mode_ok<SynPart> && SynPart::low && SynPart::part && !SynLow::part);
// the fields behind the sample clips lie where a further kernel argument of their own would: the kernels' argument loads do not move
static_assert(sizeof(SynSamples) == sizeof(UlcxSampArg) && offsetof(SynPlanes<true>, coef) == sizeof(UlcxSampArg) && offsetof(SynLow, BSw) == sizeof(UlcxSampArg));
// S coefficients at src (16-byte aligned, read once) into the padded array A; thread t0 of `step`.  DPS 4: four floats at a
// multiple of four never straddle a padding gap (spec_ld4).  The padding itself is never read by the transform.
__device__ __forceinline__ void plane_unit(float *A, const float *__restrict__ src, int S, int t0, int step) {
    static_assert(DPS == 4, "plane_unit: four consecutive floats stay clear of the padding gaps");
    for (int i = 4 * t0; i < S; i += 4 * step) {
        const f32x4 v = __builtin_nontemporal_load((const f32x4 *)(src + i));
        float *d = A + padf(i);
        *(float2 *)d = make_float2(v.x, v.y); *(float2 *)(d + 2) = make_float2(v.z, v.w);
    }
}
// The rows of a synth call, one lane per (row, per-block row) - what a walk would have left for the RANGE synthesis, from the
// caller's window codes alone.  wc [n][nPl] is not trusted: a code is taken when ulcx_window_subblocks accepts it (the codes a
// block can carry, ulcDecoder.c:211-216: 0 .. 0xFF, the second nybble only behind a first with bit 3 set), every other int32
// becomes 0, the mark of a corrupt block - the row ends there.  Nothing is drawn (draws 0), a live row's size is 1 (bitsOut
// then carries the caller's `live`), the row is entered as a range is: {1 = row 0 holds the block in front, generator state 0}.
// Without WARM row 0 is empty and the planes sit in rows 1 .. K-1, as in a range call from block 0.
__global__ __launch_bounds__(64) void k_synth_rows(int n, int K, int nPl, const int32_t *wc, int *wcScan, int *draws, int *bits, int2 *rInfo,
                                                   int32_t *skip, int32_t *len, int lenAll) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    if (id >= (long long)n * K) return;
    const int s = (int)(id / K), r = (int)(id - (long long)s * K);
    const int p = r - (K - nPl);
    int w = p >= 0 ? wc[(size_t)s * nPl + p] : 0;
    const bool ok = w > 0 && w <= 0xFF && ((w & 8) || (w >> 4) == 1);
    w = ok ? w : 0;
    wcScan[id] = w; draws[id] = 0; bits[id] = ok ? 1 : 0;
    if (r == 0) { rInfo[s] = make_int2(nPl == K ? 1 : 0, 0); skip[s] = 0; len[s] = lenAll; }
}

// LDS carve, in floats.  Stereo kernel (k_dsyn):  z [2 padded arrays of BS/2 complex] | twl [BS/4 complex] |
//   per wave: noise runs, prefix counts, seed table | 128 block / unit seeds.  General kernel (k_dgen): z [1 array] | per-wave lists.
#define DSYN_CHUNK 32            // blocks of a stream whose RNG states and headers the stereo kernel stages at once (<= 64)
struct DsynLds { int zFloats, twFloats, listFloats; };
// twInLds: the stereo kernel's FFT twiddles resident in LDS (BlockSize <= 2048; above it they are read from the tables in
// global memory, L1/L2-hot: a fourth workgroup per CU).  The lapping state is in global memory for every geometry.
// listBS: the BlockSize the per-wave lists are sized by (the low-rate source mode: the walk's; 0: BS)
// oneWave: the one-wave kernel of a stereo part call (k_dpart): z [1 array] | twl as the stereo kernel's | one wave's lists
__host__ __device__ static inline DsynLds dsyn_lds(int BS, int fast, int twInLds, int listBS = 0, int oneWave = 0) {
    DsynLds l;
    l.zFloats = (fast && !oneWave ? 2 : 1) * 2 * FFT_PADDEDS(BS / 2, DPS);
    l.twFloats = (fast && BS <= 2048 && twInLds) ? BS / 2 : 0;
    if (fast && oneWave) { l.listFloats = 64 + DSYN_PWORDS(listBS ? listBS : BS); return l; }
    l.listFloats = 2 * (64 + DSYN_PWORDS(listBS ? listBS : BS)) + 128;             // per wave: prefix counts, sign-parity stream; per workgroup: 128 block / channel RNG states
    if (fast) l.listFloats += 2 * (DSYN_CHUNK + 4) * 8;          // stereo kernel: the headers of a chunk of blocks + of a decimated block's four units, per channel
    return l;
}

// ---------------------------------------------------------------------------
// Stereo streams (BlockSize <= 4096): one workgroup = one stream, one wave per channel up to the end of the FFTs.
// ---------------------------------------------------------------------------
// The lapping state lives in global memory (L2-hot: every element is re-read by the thread that wrote it one block earlier);
// TWL: FFT twiddles in LDS (BlockSize <= 2048)
// BSC: BlockSize as a compile-time constant (2048: the headline geometry - the loops of an un-decimated block unroll, the
// table and lapping-state loads of a thread's trips can be issued together; 0: read from the context)
// MODE: the synthesis mode (above).  SynWhole: the index arithmetic and the choice of the lapping rows below fold away.  The range
// modes (SynRange and on; a cut for every grid): a stream is entered from nothing instead of from its persistent state - zero
// lapping state, the generator state the block index holds, and - unless the range starts at block 0 - the block in front of it
// (row k0 - 1 of the stream) run without output, as a cut enters a stream.  The sample store modes (SynSamples and on): every store
// of output samples goes through the (row, block)'s SampBlk instead of to the block's interleaved row.
template <typename OUT, int DEC_MAXT, bool TWL, int BSC, typename MODE>
__global__ __launch_bounds__(WG, 3) void k_dsyn(UlcxDecCtx c, MODE mode) {
    constexpr bool SPLIT = MODE::split, RANGE = MODE::range, SAMP = MODE::samp, PLANE = MODE::plane, LR = MODE::lr, LOW = MODE::low;
    extern __shared__ float lds[];
    const int BS = BSC ? BSC : c.BS, H2 = BS / 2;
    const int PW = syn_pwords(mode, BS);
    constexpr int C = 2;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const DsynLds L = dsyn_lds(BS, 1, TWL);
    float2 *z    = (float2 *)lds;
    // lapping state, in global memory: the arrays a stream's state is read from / written to at its first / last block of
    // the launch, the workgroup's own scratch rows in between.  Every element is read and rewritten by the same thread in
    // un-decimated blocks and by the same wave in decimated ones; the barriers between the two kinds of block order the rest.
    // (one workgroup per stream - grid = streams -: the stream's own rows serve, nothing else touches them during the launch)
    // (a cut launch: the leading workgroups still take one whole stream each and use its rows; the others their own scratch rows)
    const bool ownStream = !SPLIT || (int)blockIdx.x < c.synFull;
    float  *scr = ownStream ? c.lapO + (size_t)(c.s0 + blockIdx.x) * C * H2 : c.lapScratch + (size_t)((int)blockIdx.x - c.synFull) * C * H2;
    float2 *twl  = (float2 *)(lds + L.zFloats);        // FFT twiddles: the full-size table, or the three of a decimated block's sizes
    SynWave sw;
    sw.pre  = (int *)(lds + L.zFloats + L.twFloats) + wv * (64 + PW);
    sw.seedTab = (uint32_t *)(sw.pre + 64);
    uint32_t *bseed = (uint32_t *)(lds + L.zFloats + L.twFloats + 2 * (64 + PW));   // [0,64): RNG state at each block's start, [64,128): at its second channel
    // [wave][block of the chunk][8]: {window code, the first unit's four record fields, its draws (un-decimated block), its tail decay, -}
    int *hdr = (int *)(bseed + 128) + wv * ((DSYN_CHUNK + 4) * 8);
    sw.lane = lane;
    if (TWL) for (int i = tid; i < BS / 4; i += WG) twl[i] = c.T.tw[0][i];
    bool twFull = true;
    const int M0 = BS >> 1, Mp0 = FFT_PADDEDS(M0, DPS);
    float2 *zc = z + wv * Mp0;                                       // this wave's channel
#ifdef ULCX_DSYN_STAMPS
    // diagnostic build only: shader cycles per phase, summed over the workgroup's blocks
    DsynStamps stq; for (int i = 0; i < DSYN_NSTAMP; i++) stq.t[i] = 0; stq.t0 = __builtin_amdgcn_s_memtime();
    sw.stp = &stq;
#define STAMP(i) do { unsigned long long t_ = __builtin_amdgcn_s_memtime(); stq.t[i] += t_ - stq.t0; stq.t0 = t_; } while (0)
#else
#define STAMP(i) do {} while (0)
#endif
    __syncthreads();

    // The (stream, block) pairs of the launch in stream-major order, cut evenly over the grid (round 3).  One workgroup
    // per stream is the special case grid = streams.  A workgroup that enters a stream behind its first block of the
    // launch runs the block in front of its range without output first: the lapping state a block leaves depends on that
    // block alone (the pending list is rewritten in full: dec_time_wave, and the un-decimated epilogue below), the RNG
    // state is reached by a jump over the draws of the blocks in front, LastSubBlockSize follows from the previous
    // block's window code.  So 4096 streams need not come in rounds of the machine's 1536 workgroup slots (2.67 rounds,
    // the last one a third full), and a few long streams fill the machine too.
    const int Kc = c.k1 - c.k0;
    const long long T = (long long)(c.s1 - c.s0) * Kc;
    long long f0 = (long long)blockIdx.x * Kc, f1 = f0 + Kc;
    if (!ownStream) {
        const long long base = (long long)c.synFull * Kc, Tr = T - base;
        const int j = (int)blockIdx.x - c.synFull, n = (int)gridDim.x - c.synFull;
        f0 = base + Tr * j / n; f1 = base + Tr * (j + 1) / n;
    }
    if (f0 >= f1) return;
    bool warm = SPLIT && (f0 % Kc) != 0;
    int nTrip = (int)(f1 - f0) + (warm ? 1 : 0);
    int s = c.s0 + (int)((f0 - (warm ? 1 : 0)) / Kc), k = c.k0 + (int)((f0 - (warm ? 1 : 0)) % Kc) - 1;
    if constexpr (RANGE) {
        if (f0 % Kc == 0) {                                          // at a stream's start: its block in front first, if it has one
            const int pre = c.rInfo[s].x;
            warm = pre != 0; nTrip += pre; k -= pre;
        }
    }
    int sCur = -1, lastSub = 0, dead = 0, chunkK = -1;
    uint32_t seed = 0;
    int rowSkip = 0, rowLen = 0;                                     // SAMP: the row's first sample within its first block, its length
    const int laneOuter = lane, tidOuter = tid;
    for (; nTrip > 0; nTrip--, warm = false) {
        // Inside this loop over the blocks the compiler hoists every load and index that depends on the thread only
        // (pre-twiddles, window factors, bit-reversed positions, padded FFT addresses) out of the loop - registers held
        // across all blocks.  Opaque copies of the thread's indices keep them where they are used.
        int lane = laneOuter, tid = tidOuter;
        asm volatile("" : "+v"(lane), "+v"(tid));
        sw.lane = lane;                                              // (round 3: 168 registers with spills -> 156 without, 1.05 -> 1.00 ms)
        if (++k == c.k1) {
            k = c.k0; s++;
            if constexpr (RANGE) { if (c.rInfo[s].x) { k = c.k0 - 1; warm = true; nTrip++; } }
        }
        const int blk = s * c.K + k;
        if (s != sCur) {
            // entering a stream, at its first block of the launch or behind it: the state in front of block k
            sCur = s;
            __syncthreads();
            int bad = 0; uint32_t dsum = 0;
            const int kf = RANGE ? c.k0 - c.rInfo[s].x : c.k0;       // the stream's first row of the launch
            for (int j = kf + tid; j < k; j += WG) {                 // blocks of the launch in front of k (none at the stream's start)
                const int bj = s * c.K + j;
                if (c.wcScan[bj] == 0) bad = 1;
                if constexpr (!PLANE) dsum += (uint32_t)c.draws[bj];
            }
            bad = __syncthreads_or(bad);
            dead = RANGE ? bad : (c.dead[s] | bad);                  // (a corrupt block in front: the stream is dead, no other state matters)
            lastSub = RANGE ? 0 : c.lastSub[s];
            if constexpr (!PLANE) seed = RANGE ? (uint32_t)c.rInfo[s].y : c.seed[s];
            if constexpr (SAMP) { rowSkip = mode.s.skip[s]; rowLen = mode.s.len[s]; }
            if constexpr (RANGE) { if (k == c.k0 && kf == c.k0) for (int i = tid; i < 2 * H2; i += WG) scr[i] = 0.0f; }   // a range from block 0: nothing pending (ordered by the barrier in front of the chunk's tables)
            if (k > kf) {
                if constexpr (!PLANE) {
                const uint32_t ws = wave_scan_add(dsum);             // (lane 63: the wave's sum)
                if (lane == 63) bseed[wv] = ws;
                __syncthreads();
                seed = rng_jump(c.jumpT, seed, bseed[0] + bseed[1]);
                __syncthreads();
                }
                lastSub = last_sub_size(BS, c.wcScan[blk - 1]);              // as block k-1 left it
            }
            chunkK = -1;
        }
        if (chunkK < 0 || k >= chunkK + DSYN_CHUNK) {
            // The stream's one RNG chain (ulcDecoder.c:75-81) for the next DSYN_CHUNK blocks at once: a block starts draws-
            // of-its-predecessors after the chunk's first state - one lane per block, prefix sum, one jump each (wave 1: the
            // state at each block's second channel).  A corrupt block ends the stream: it and its successors draw nothing.
            // The same lanes leave what a block's first unit needs from the walk's per-block arrays in LDS: a block
            // then starts from LDS instead of from a round trip to HBM.
            __syncthreads();
            const int kk = k + lane, bk = s * c.K + (kk < c.k1 && lane < DSYN_CHUNK ? kk : k);
            const bool on = kk < c.k1 && lane < DSYN_CHUNK;
            const int wcl = c.wcScan[bk];
            if constexpr (PLANE) {                                   // the chunk's tables keep the window codes only
                if (lane < DSYN_CHUNK) hdr[lane * 8] = wcl;
                __syncthreads();
            } else {
            const int drb = c.draws[bk];
            const int ud4 = c.unitDraws[(size_t)bk * C * 4 + 4];
            const int4 url = c.unitRec[(size_t)bk * C * 4 + wv * 4];
            const float rrl = c.unitTail[(size_t)bk * C * 4 + wv * 4].y;
            int dr = on ? drb : 0;
            const unsigned long long badm = __ballot(on && wcl == 0);
            if (badm && lane >= __builtin_ctzll(badm)) dr = 0;
            const uint32_t incl = wave_scan_add((uint32_t)dr);
            const uint32_t before = incl - (uint32_t)dr + (wv ? (uint32_t)ud4 : 0u);
            bseed[wv * 64 + lane] = rng_jump(c.jumpT, seed, before);
            if (lane < DSYN_CHUNK) {
                int *h = hdr + lane * 8;
                h[0] = wcl; h[1] = url.x; h[2] = url.y; h[3] = url.z; h[4] = url.w;
                h[5] = wv ? drb - ud4 : ud4;                       // draws of the channel's one unit in an un-decimated block (unitDraws[0] = 0)
                h[6] = __float_as_int(rrl);
            }
            const uint32_t chunkDraws = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            __syncthreads();
            seed = rng_jump(c.jumpT, seed, chunkDraws);            // state after the chunk: the next chunk's start / the stream's state behind the launch
            }
            chunkK = k;
        }
        const int kb = k - chunkK;                                   // this block's slot in the chunk's tables
        const int *hb = hdr + kb * 8;
        const int wc = hb[0];
        if (wc == 0) dead = 1;                                       // a corrupt block ends the stream (ulcDecodeTool.c:154-157)
        const bool lastOfStream = k == c.k1 - 1;
        const size_t oblk = RANGE ? (size_t)s * (c.K - 1) + (warm ? 0 : k - 1) : (size_t)blk;   // (a range call's output has no row for the block in front)
        OUT *outp = out_base<OUT>(c) + oblk * C * BS;
        SampBlk<OUT> sb; OUT *sp0 = nullptr, *sp1 = nullptr; bool sal0 = false, sal1 = false;   // SAMP: where this block's samples go instead - the two planes, and whether their pairs are aligned
        if constexpr (SAMP) {
            sb = samp_blk<OUT>(out_base<OUT>(c), C, BS, mode.s.nSamples, s, warm ? 0 : k - 1, rowSkip, rowLen);
            sp0 = sb.plane(0); sp1 = sb.plane(1); sal0 = sb.pairs(sp0); sal1 = sb.pairs(sp1);
        }
        if constexpr (RANGE) { if (!warm && tid == 0) c.bitsOut[oblk] = dead ? 0 : c.bits[blk]; }
        // where this block finds and leaves the lapping state
        const float *lapR = (!SPLIT || RANGE) ? scr : (k == c.k0 ? c.lap + (size_t)s * C * H2 : scr);
        float *lapW = !SPLIT ? scr : (lastOfStream ? c.lapO + (size_t)s * C * H2 : scr);
        if (dead) {
            if (!warm) {
                if constexpr (SAMP) sb.zero(C, tid);
                else for (int i = tid; i < C * BS; i += WG) st1(outp + i, 0.0f);
                if (tid == 0) c.bits[blk] = 0;
            }
            if (lastOfStream && tid == 0) { c.lastSubO[s] = lastSub; c.seedO[s] = seed; c.deadO[s] = 1; }
            if (lastOfStream) for (int i = tid; i < 2 * H2; i += WG) lapW[i] = 0.0f;     // (never read again: the stream stays dead)
            continue;
        }
        const int *udraw = c.unitDraws + (size_t)blk * C * 4;
        const int4 *urec = c.unitRec + (size_t)blk * C * 4;
        const float4 *utail = c.unitTail + (size_t)blk * C * 4;
        const uint2 *prec = c.prec + (size_t)blk * c.precStride, *nrec = c.nrec + (size_t)blk * c.nrecStride;
        const float *tmag = c.tailMag + (size_t)blk * C * 4 * c.tailStride;
        const BlockShape shape = block_shape(BS, wc);
        const unsigned pat0 = shape.pat;
        const bool whole = shape.whole;
        const int nsub = shape.nsub;
        if (TWL && whole != twFull) {
            // twiddle tables for this block's transform sizes: the full-size one, or those of N/2, N/4, N/8 back to back
            if (whole) for (int i = tid; i < BS / 4; i += WG) twl[i] = c.T.tw[0][i];
            else for (int i = tid; i < 7 * BS / 32; i += WG) {
                const int dd = i < BS / 8 ? 1 : i < 3 * BS / 16 ? 2 : 3;
                twl[i] = c.T.tw[dd][i - (dd == 1 ? 0 : dd == 2 ? BS / 8 : 3 * BS / 16)];
            }
            twFull = whole;
            __syncthreads();
        }
        STAMP(0);
        // Decimated block (round 5): what its 2..4 units need from the walk - record ranges, draws, tail decay - and their RNG start
        // states (a table jump of up to four dependent look-ups each) are fetched for ALL units at once, unit j in lane j, and
        // handed out by lane reads; a unit used to start with its own loads and its own jump, one after the other.
        int *uh = hdr + DSYN_CHUNK * 8;                              // [4 units][8] of this wave, behind its chunk table
        const float *plane = nullptr;                                // PLANE: this wave's channel of the block, where the records' place is
        if constexpr (PLANE) plane = mode.unit(s, C, wv, c.K, k, BS);
        if (!PLANE && !whole) {
            if (lane < nsub) {
                const int dj = udraw[wv * 4 + lane];
                const int dn = (lane + 1 < nsub) ? udraw[wv * 4 + lane + 1] : (wv + 1 < C) ? udraw[(wv + 1) * 4] : c.draws[blk];
                const int4 urL = urec[wv * 4 + lane];
                const float rrL = utail[wv * 4 + lane].y;
                const uint32_t seedL = rng_jump(c.jumpT, bseed[kb], (uint32_t)dj);
                int *u = uh + lane * 8;
                u[0] = (int)seedL; u[1] = urL.x; u[2] = urL.y; u[3] = urL.z; u[4] = urL.w; u[5] = dn - dj; u[6] = __float_as_int(rrL);
            }
            WAVE_SYNC();
        }
        // ---- coefficients -> spectra, this wave's channel, subblock by subblock (independent of each other)
        {
            unsigned pat = pat0; int off = 0;
            for (int j = 0; j < nsub; j++, pat >>= 4) {
                const int d = pat & 7, S = BS >> d, M = S >> 1, Mp = FFT_PADDEDS(M, DPS);
                float2 *zj = zc + FFT_PADS(off >> 1, DPS);
                sw.A = (float *)zj;
                if constexpr (PLANE) {
                    // the unit's coefficients from the caller's plane, where synth_unit sits: in flight beside the other wave's transform
                    plane_unit((float *)zj, plane + off, S, lane, 64);
                    WAVE_SYNC();
                } else {
                const int *uj = uh + j * 8;
                const uint32_t unitSeed = whole ? bseed[wv * 64 + kb] : (uint32_t)uj[0];
                STAMP(1);
                const int4 ur = whole ? make_int4(hb[1], hb[2], hb[3], hb[4]) : make_int4(uj[1], uj[2], uj[3], uj[4]);
                const int ud = whole ? hb[5] : uj[5];
                const float urr = __int_as_float(whole ? hb[6] : uj[6]);
                if (!(ULCX_DBG(c) & 1)) synth_unit<LOW>(c, sw, S, prec, nrec, ur, unitSeed, ud, urr, tmag + (size_t)(wv * 4 + j) * c.tailStride, Mp);
                else for (int i = lane; i < Mp; i += 64) zj[i] = make_float2(0.0f, 0.0f);
                }
                STAMP(2);

                // DCT-IV pre-twiddle in place: n and M-1-n together read and write the same two complex slots
                const float2 *pre = c.T.pre[d];
                if (!(ULCX_DBG(c) & 2)) {
                if (BSC == 2048 && whole) {
                    // the headline geometry: eight trips per lane, four at a time with every load of the four in front of the
                    // arithmetic (a trip is a chain load -> multiply -> store; in a loop the eight chains run one after the other)
                    constexpr int MC = 1024;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        float2 va[4], vb[4], p1[4], p2[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            const int n = lane + 64 * (4 * h + t), n2 = MC - 1 - n;
                            va[t] = zj[FFT_PADS(n, DPS)]; vb[t] = zj[FFT_PADS(n2, DPS)]; p1[t] = pre[n]; p2[t] = pre[n2];
                        }
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            const int n = lane + 64 * (4 * h + t), n2 = MC - 1 - n;
                            zj[FFT_PADS(n, DPS)]  = cmulc(make_float2(va[t].x, vb[t].y), p1[t]);
                            zj[FFT_PADS(n2, DPS)] = cmulc(make_float2(vb[t].x, va[t].y), p2[t]);
                        }
                    }
                } else {
#pragma unroll
                for (int n = lane; n < M / 2; n += 64) {
                    const int n2 = M - 1 - n;
                    const int pn = FFT_PADS(n, DPS), pn2 = FFT_PADS(n2, DPS);
                    const float2 a = zj[pn], b = zj[pn2];            // (X[2n], X[2n+1]), (X[S-2-2n], X[S-1-2n])
                    zj[pn]  = cmulc(make_float2(a.x, b.y), pre[n]);
                    zj[pn2] = cmulc(make_float2(b.x, a.y), pre[n2]);
                }
                }
                STAMP(11);
                if constexpr (!TWL) { if (M == 1024) fft_wave_dif_ct<1024, DPS>(zj, c.T.tw[d], lane); else fft_wave_dif(zj, M, c.T.tw[d], lane, DPS); }
                else if (M == 1024) fft_wave_dif_ct<1024, DPS>(zj, twl, lane);     // (BlockSize 2048, un-decimated: index arithmetic folded at compile time)
                else fft_wave_dif(zj, M, twl + (d <= 1 ? 0 : d == 2 ? BS / 8 : 3 * BS / 16), lane, DPS);
                }
                STAMP(3);
                off += S;
            }
        }
        if (whole) {
            // ---- un-decimated block (the common case), both channels together: post-twiddle fused with the windowed
            //      overlap-add (oracle/orc_fourier.c orc_imdct), inverse M/S in registers, interleaved stores
            int ov = BS;                                             // ulcDecoder.c:234-239
            if (pat0 & 8) ov >>= (wc & 7);
            if (ov > lastSub) ov = lastSub;
            if constexpr ((BSC == 2048 || BSC == 4096) && DSYN_EPI2) {
                // Headline geometry and BlockSize 4096 (round 5): a two-deep pipeline over the thread's four (eight) trips.  What a trip reads from global
                // memory (two post-twiddles, the pending halves of both channels, the window pair: 12 registers) is asked for one
                // trip ahead - the first trip's BEFORE the barrier, where the transform's registers are free and the other
                // wave may still be transforming.  (All four at once spill: 1.70 -> 1.89 ms.)  Window pair: p1 = p0 - 1 is even
                // and so are a and ov: aligned 8-byte loads; below the ramp the index is clamped, the value unused.
                constexpr int S = BSC, M = BSC / 2, NT = M / 2 / WG;
                const float2 *pre = c.T.pre[0];
                const float2 *z0 = z, *z1 = z + Mp0;
                const int a = (S - ov) >> 1;
                const float *fall = c.T.winFall + ov, *rise = c.T.winRise + ov;
                float *L0 = lapW, *L1 = lapW + H2;
                struct Ops { float2 P1, P2, Am, As, F, R; };
                auto fetch = [&](int t) {
                    Ops o;
                    const int k1 = tid + WG * t, k2 = M - 1 - k1;
                    o.P1 = pre[k1]; o.P2 = pre[k2];
                    o.Am = make_float2(0.0f, 0.0f); o.As = o.Am; o.F = o.Am; o.R = o.Am;
                    if (!warm) {
                        o.Am = *(const float2 *)(lapR + 2 * k1); o.As = *(const float2 *)(lapR + H2 + 2 * k1);
                        int wi = M - 2 - 2 * k1 - a; wi = wi < 0 ? 0 : wi;
                        o.F = *(const float2 *)(fall + wi); o.R = *(const float2 *)(rise + wi);
                    }
                    return o;
                };
                // The 8-byte window loads want a, ov and p1 even: ov = BS >> (0..7) capped by lastSub >= BS / 8, both multiples of 4
                // for every BlockSize this branch is compiled for (>= 2048), so a = (S - ov) / 2 is even too.
                static_assert(BSC >= 2048 && (BSC >> 7) % 4 == 0 && (BSC >> 3) % 4 == 0, "k_dsyn: the pipelined epilogue loads window pairs as float2");
                Ops nxt = fetch(0);
                __syncthreads();
                STAMP(4);
                if (!(ULCX_DBG(c) & 4))                             // (ablation builds only: the epilogue skipped, as in the generic loop below)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const Ops cur = nxt;
                    if (t + 1 < NT) nxt = fetch(t + 1);
                    const int k1 = tid + WG * t, k2 = M - 1 - k1;
                    constexpr int LGM = BSC == 4096 ? 11 : 10;
                    int r1 = (int)(__brev((unsigned)k1) >> (32 - LGM)), r2 = (int)(__brev((unsigned)k2) >> (32 - LGM));
                    r1 = FFT_PADS(r1, DPS); r2 = FFT_PADS(r2, DPS);
                    const float2 ya1 = cmulc_post(z0[r1], cur.P1), ya2 = cmulc_post(z0[r2], cur.P2);     // channel 0 (M): (Re y, -Im y)
                    const float2 yb1 = cmulc_post(z1[r1], cur.P1), yb2 = cmulc_post(z1[r2], cur.P2);     // channel 1 (S)
                    if (!warm) {
                        const float Bm[2] = { ya1.y, ya2.x }, Bs[2] = { yb1.y, yb2.x };
                        const float Am[2] = { cur.Am.x, cur.Am.y }, As[2] = { cur.As.x, cur.As.y };
                        const float Fw[2] = { cur.F.y, cur.F.x }, Rw[2] = { cur.R.y, cur.R.x };        // (the pair is {p1, p0})
                        const int   pv[2] = { M - 1 - 2 * k1, M - 2 - 2 * k1 };
                        float2 lo2[2], hi2[2];
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            float mLo, mHi, sLo, sHi;
                            if (pv[q] < a) { mLo = Am[q]; mHi = Bm[q]; sLo = As[q]; sHi = Bs[q]; }
                            else {
                                const float cw = Fw[q], sn = Rw[q];
                                const float m1 = sn * Bm[q], m3 = cw * Bm[q];
                                mLo = __builtin_fmaf(cw, Am[q], -m1); mHi = __builtin_fmaf(sn, Am[q], m3);
                                const float s1 = sn * Bs[q], s3 = cw * Bs[q];
                                sLo = __builtin_fmaf(cw, As[q], -s1); sHi = __builtin_fmaf(sn, As[q], s3);
                            }
                            if constexpr (LR) { lo2[q] = make_float2(mLo, sLo); hi2[q] = make_float2(mHi, sHi); }
                            else {
                            lo2[q] = make_float2(mLo + sLo, mLo - sLo);
                            hi2[q] = make_float2(mHi + sHi, mHi - sHi);
                            }
                        }
                        if constexpr (SAMP) {
                            sb.two(sp0, sal0, pv[1], lo2[1].x, lo2[0].x); sb.two(sp1, sal1, pv[1], lo2[1].y, lo2[0].y);
                            sb.two(sp0, sal0, S - 1 - pv[0], hi2[0].x, hi2[1].x); sb.two(sp1, sal1, S - 1 - pv[0], hi2[0].y, hi2[1].y);
                        } else {
                        st4(outp + 2 * pv[1], lo2[1].x, lo2[1].y, lo2[0].x, lo2[0].y);
                        st4(outp + 2 * (S - 1 - pv[0]), hi2[0].x, hi2[0].y, hi2[1].x, hi2[1].y);
                        }
                    }
                    *(float2 *)(L0 + 2 * k1) = make_float2(ya1.x, ya2.y);
                    *(float2 *)(L1 + 2 * k1) = make_float2(yb1.x, yb2.y);
                }
            } else {
            __syncthreads();
            STAMP(4);
            if (!(ULCX_DBG(c) & 4)) {
                const int S = BS, M = M0;
                const float2 *pre = c.T.pre[0];
                const float2 *z0 = z, *z1 = z + Mp0;
                const int a = (S - ov) >> 1;
                const float *fall = c.T.winFall + ov, *rise = c.T.winRise + ov;
                const int bits = 31 - __clz(M);
                const float *R0 = lapR, *R1 = lapR + H2;
                float *L0 = lapW, *L1 = lapW + H2;
#pragma unroll
                for (int kk = tid; kk < M / 2; kk += WG) {
                    const int k1 = kk, k2 = M - 1 - kk;
                    int r1 = (int)(__brev((unsigned)k1) >> (32 - bits));
                    int r2 = (int)(__brev((unsigned)k2) >> (32 - bits));
                    r1 = FFT_PADS(r1, DPS); r2 = FFT_PADS(r2, DPS);
                    const float2 P1 = pre[k1], P2 = pre[k2];
                    const float2 ya1 = cmulc_post(z0[r1], P1), ya2 = cmulc_post(z0[r2], P2);     // channel 0 (M): (Re y, -Im y)
                    const float2 yb1 = cmulc_post(z1[r1], P1), yb2 = cmulc_post(z1[r2], P2);     // channel 1 (S)
                    if (!warm) {
                    const float A0m = R0[2 * k1], A1m = R0[2 * k1 + 1], A0s = R1[2 * k1], A1s = R1[2 * k1 + 1];
                    const float Bm[2] = { ya1.y, ya2.x }, Bs[2] = { yb1.y, yb2.x };
                    const float Am[2] = { A0m, A1m }, As[2] = { A0s, A1s };
                    const int   pv[2] = { M - 1 - 2 * k1, M - 2 - 2 * k1 };
                    float2 lo2[2], hi2[2];                                             // interleaved L/R at positions p and S-1-p
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int p = pv[q];
                        const bool pass = p < a;
                        float cw = 0.0f, sn = 0.0f;
                        if (!pass) { cw = fall[p - a]; sn = rise[p - a]; }
                        const LapPair m = lap_pair(Am[q], Bm[q], cw, sn, pass), sd = lap_pair(As[q], Bs[q], cw, sn, pass);   // outputs at positions p and S-1-p
                        // inverse M/S (ulcDecoder.c:281-289) + interleave (:292-297)
                        if constexpr (LR) { lo2[q] = make_float2(m.lo, sd.lo); hi2[q] = make_float2(m.hi, sd.hi); }
                        else {
                        lo2[q] = make_float2(m.lo + sd.lo, m.lo - sd.lo);
                        hi2[q] = make_float2(m.hi + sd.hi, m.hi - sd.hi);
                        }
                    }
                    // positions pv[1] = pv[0]-1 and S-1-pv[0], S-pv[0] are neighbours: two aligned 16-byte stores
                    if constexpr (SAMP) {
                        sb.two(sp0, sal0, pv[1], lo2[1].x, lo2[0].x); sb.two(sp1, sal1, pv[1], lo2[1].y, lo2[0].y);
                        sb.two(sp0, sal0, S - 1 - pv[0], hi2[0].x, hi2[1].x); sb.two(sp1, sal1, S - 1 - pv[0], hi2[0].y, hi2[1].y);
                    } else {
                    st4(outp + 2 * pv[1], lo2[1].x, lo2[1].y, lo2[0].x, lo2[0].y);
                    st4(outp + 2 * (S - 1 - pv[0]), hi2[0].x, hi2[0].y, hi2[1].x, hi2[1].y);
                    }
                    }
                    L0[2 * k1] = ya1.x; L0[2 * k1 + 1] = ya2.y;
                    L1[2 * k1] = yb1.x; L1[2 * k1 + 1] = yb2.y;
                }
            }
            }
            STAMP(5);
            __syncthreads();
            STAMP(6);
            lastSub = BS;
        } else {
            // ---- decimated block: each wave finishes its channel in LDS, then both channels together:
            //      inverse M/S (ulcDecoder.c:281-289) + interleave (:292-297)
            // (the time-domain pass works on the lapping state in place: in the workgroup's own rows)
            if (lapR != scr && !warm) { for (int i = tid; i < 2 * H2; i += WG) scr[i] = lapR[i]; __syncthreads(); }
            WAVE_SYNC();
            const int newLast = dec_time_wave<DEC_MAXT>(c, zc, scr + wv * H2, wc, pat0, nsub, lastSub, lane);
            __syncthreads();
            // output = times [-BS/2, BS/2) of both channels: the old pending lists (time -1-i at lap[i]), then the arrays
            const float *t0 = (const float *)z, *t1 = (const float *)(z + Mp0);
            const float *L0 = scr, *L1 = scr + H2;
            if (!warm) {
            for (int n = 2 * tid; n < H2; n += 2 * WG) {
                const float mx = L0[H2 - 1 - n], my = L0[H2 - 2 - n], sx = L1[H2 - 1 - n], sy = L1[H2 - 2 - n];
                if constexpr (LR) { sb.two(sp0, sal0, n, mx, my); sb.two(sp1, sal1, n, sx, sy); }
                else if constexpr (SAMP) { sb.two(sp0, sal0, n, mx + sx, my + sy); sb.two(sp1, sal1, n, mx - sx, my - sy); }
                else st4(outp + 2 * n, mx + sx, mx - sx, my + sy, my - sy);
            }
            for (int n = 2 * tid; n < H2; n += 2 * WG) {
                const float2 m = *(const float2 *)(t0 + padf(n)), sd = *(const float2 *)(t1 + padf(n));
                if constexpr (LR) { sb.two(sp0, sal0, H2 + n, m.x, m.y); sb.two(sp1, sal1, H2 + n, sd.x, sd.y); }
                else if constexpr (SAMP) { sb.two(sp0, sal0, H2 + n, m.x + sd.x, m.y + sd.y); sb.two(sp1, sal1, H2 + n, m.x - sd.x, m.y - sd.y); }
                else st4(outp + 2 * (H2 + n), m.x + sd.x, m.x - sd.x, m.y + sd.y, m.y - sd.y);
            }
            }
            __syncthreads();
            // new pending lists: times [BS/2, BS) of the arrays
            for (int i = tid; i < 2 * H2; i += WG) {
                const int ch = i >= H2 ? 1 : 0, m = i - ch * H2;
                lapW[ch * H2 + H2 - 1 - m] = ((const float *)(z + ch * Mp0))[padf(H2 + m)];
            }
            __syncthreads();
            lastSub = newLast;
            STAMP(7);
        }
        if (lastOfStream && tid == 0) { c.lastSubO[s] = lastSub; c.seedO[s] = seed; c.deadO[s] = dead; }
    }
#ifdef ULCX_DSYN_STAMPS
    if (lane == 0) for (int i = 0; i < DSYN_NSTAMP; i++) ((unsigned long long *)(c.scratch + (size_t)s * 4 * BS))[wv * DSYN_NSTAMP + i] = stq.t[i];
#endif
}

// ---------------------------------------------------------------------------
// Everything else (mono / multichannel / BlockSize > 4096): one (channel, subblock) at a time through ONE LDS array,
// the lapping state and the staging of the time samples in global memory.  Correct for every geometry the
// reference accepts (ulcDecoder.c:33-35: up to 255 channels, BlockSize up to 32768), not tuned.
// ---------------------------------------------------------------------------
// MODE: the synthesis mode, as k_dsyn's; one workgroup per stream whatever its `split` says.
template <typename OUT, typename MODE>
__global__ __launch_bounds__(WG) void k_dgen(UlcxDecCtx c, MODE mode) {
    constexpr bool RANGE = MODE::range, SAMP = MODE::samp, PLANE = MODE::plane, LR = MODE::lr, LOW = MODE::low, PART = MODE::part;
    extern __shared__ float lds[];
    const int BS = c.BS, C = c.C, H2 = BS / 2;
    // PART: the coded channels ch0, ch0 + 2, ... alone, channel ch into plane ch >> 1 of CO; the records, draws and the lapping rows stay indexed by ch
    int ch0 = 0, chStep = 1, CO = C;
    if constexpr (PART) { ch0 = mode.which; chStep = 2; CO = mode.nOut; }
    const int s = c.s0 + blockIdx.x, tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const DsynLds L = dsyn_lds(BS, 0, 0);
    float2 *z = (float2 *)lds;
    SynWave sw;
    sw.pre  = (int *)(lds + L.zFloats) + wv * (64 + syn_pwords(mode, BS));
    sw.seedTab = (uint32_t *)(sw.pre + 64);
    sw.lane = lane;
#ifdef ULCX_DSYN_STAMPS
    sw.stp = nullptr;
#endif
    float *glap = c.lap + (size_t)s * C * H2;
    int lastSub = c.lastSub[s];
    int dead = c.dead[s];
    uint32_t seed = c.seed[s];
    float *scr = c.scratch + (size_t)s * 4 * BS;                     // staging: dst[2][BS] | dec[BS] | tmpq[BS/2]
    int kBeg = 0, rowSkip = 0, rowLen = 0;
    if constexpr (SAMP) { rowSkip = mode.s.skip[s]; rowLen = mode.s.len[s]; }
    if constexpr (RANGE) {
        // a range call (k_dsyn): the stream is entered from nothing - zero lapping state, the index's generator state -, and
        // row 0, the block in front of the range, runs without output when there is one
        const int2 ri = c.rInfo[s];
        lastSub = 0; dead = 0; seed = (uint32_t)ri.y; kBeg = 1 - ri.x;
        for (int i = tid; i < C * H2; i += WG) glap[i] = 0.0f;
        __syncthreads();
    }
    for (int k = kBeg; k < c.K; k++) {
        const int blk = s * c.K + k;
        const int wc = c.wcScan[blk];
        if (wc == 0) dead = 1;                                       // a corrupt block ends the stream (ulcDecodeTool.c:154-157)
        const bool warm = RANGE && k == 0;
        const size_t oblk = RANGE ? (size_t)s * (c.K - 1) + (warm ? 0 : k - 1) : (size_t)blk;
        OUT *outp = out_base<OUT>(c) + oblk * C * BS;
        SampBlk<OUT> sb;
        if constexpr (SAMP) sb = samp_blk<OUT>(out_base<OUT>(c), PART ? CO : C, BS, mode.s.nSamples, s, warm ? 0 : k - 1, rowSkip, rowLen);
        if constexpr (RANGE) { if (!warm && tid == 0) c.bitsOut[oblk] = dead ? 0 : c.bits[blk]; }
        if (dead) {
            if constexpr (SAMP) { if (!warm) sb.zero(PART ? CO : C, tid); }
            else
            if (!warm) for (int i = tid; i < C * BS; i += WG) st1(outp + i, 0.0f);
            if (tid == 0) c.bits[blk] = 0;
            continue;
        }
        const int *udraw = c.unitDraws + (size_t)blk * C * 4;
        const int4 *urec = c.unitRec + (size_t)blk * C * 4;
        const float4 *utail = c.unitTail + (size_t)blk * C * 4;
        const uint2 *prec = c.prec + (size_t)blk * c.precStride, *nrec = c.nrec + (size_t)blk * c.nrecStride;
        const float *tmag = c.tailMag + (size_t)blk * C * 4 * c.tailStride;
        const BlockShape shape = block_shape(BS, wc);
        const unsigned pat0 = shape.pat;
        const int nsub = shape.nsub;
        auto unit_draws = [&](int ch, int j) { return ((j + 1 < nsub) ? udraw[ch * 4 + j + 1] : (ch + 1 < C) ? udraw[(ch + 1) * 4] : c.draws[blk]) - udraw[ch * 4 + j]; };
        {
            float *dec = scr + 2 * BS, *tmpq = scr + 3 * BS;
            int newLast = lastSub;
            for (int ch = PART ? ch0 : 0; ch < C; ch += PART ? chStep : 1) {
                int last = lastSub;                                  // ulcDecoder.c:219
                float *dst = scr + (size_t)(ch & 1) * BS;
                float *Lp = glap + (size_t)ch * H2;
                unsigned pat = pat0;
                int dpos = 0, j = 0;
                do {
                    const int d = pat & 7, S = BS >> d, M = S >> 1, Mp = FFT_PADDEDS(M, DPS);
                    int ov = S;                                      // ulcDecoder.c:234-239
                    if (pat & 8) ov >>= (wc & 7);
                    if (ov > last) ov = last;
                    last = S;
                    if constexpr (PLANE) plane_unit((float *)z, mode.unit(s, C, ch, c.K, k, BS) + dpos, S, tid, WG);   // the unit from the caller's plane
                    else {
                    for (int i = tid; i < Mp; i += WG) z[i] = make_float2(0.0f, 0.0f);
                    __syncthreads();
                    if (wv == 0) {
                        sw.A = (float *)z;
                        const uint32_t unitSeed = rng_jump(c.jumpT, seed, (uint32_t)udraw[ch * 4 + j]);
                        synth_unit<LOW>(c, sw, S, prec, nrec, urec[ch * 4 + j], unitSeed, unit_draws(ch, j), utail[ch * 4 + j].y, tmag + (size_t)(ch * 4 + j) * c.tailStride);
                    }
                    }
                    __syncthreads();
                    const float2 *pre = c.T.pre[d];
                    for (int n = tid; n < M / 2; n += WG) {
                        const int n2 = M - 1 - n;
                        const int pn = FFT_PADS(n, DPS), pn2 = FFT_PADS(n2, DPS);
                        const float2 a = z[pn], b = z[pn2];
                        z[pn]  = cmulc(make_float2(a.x, b.y), pre[n]);
                        z[pn2] = cmulc(make_float2(b.x, a.y), pre[n2]);
                    }
                    __syncthreads();
                    if (wv == 0) fft_wave_dif(z, M, c.T.tw[d], lane, DPS);
                    __syncthreads();
                    // post-twiddle fused with the windowed overlap (oracle/orc_fourier.c orc_imdct):
                    //   zz[2k] = Re y[k], zz[S-1-2k] = -Im y[k];  pair p: A = lap[M-1-p], B = zz[M+p]
                    float *out = (S == BS) ? dst : dec;
                    const int a = (S - ov) >> 1;
                    const float *fall = c.T.winFall + ov, *rise = c.T.winRise + ov;
                    const int bits = 31 - __clz(M);
                    for (int kk = tid; kk < M / 2; kk += WG) {
                        const int k1 = kk, k2 = M - 1 - kk;
                        const int r1 = FFT_PADS((int)(__brev((unsigned)k1) >> (32 - bits)), DPS);
                        const int r2 = FFT_PADS((int)(__brev((unsigned)k2) >> (32 - bits)), DPS);
                        const float2 y1 = cmulc_post(z[r1], pre[k1]), y2 = cmulc_post(z[r2], pre[k2]);      // (Re y, -Im y)
                        // zz[2k1] = Re y1, zz[2k1+1] = -Im y2 (new lap);  zz[S-1-2k1] = -Im y1, zz[S-2-2k1] = Re y2 (B values)
                        const float A0 = Lp[2 * k1], A1 = Lp[2 * k1 + 1];
                        const float Bv[2] = { y1.y, y2.x };
                        const float Av[2] = { A0, A1 };
                        const int   pv[2] = { M - 1 - 2 * k1, M - 2 - 2 * k1 };
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const int p = pv[q];
                            const bool pass = p < a;
                            float cw = 0.0f, sn = 0.0f;
                            if (!pass) { cw = fall[p - a]; sn = rise[p - a]; }
                            const LapPair r = lap_pair(Av[q], Bv[q], cw, sn, pass);
                            out[p] = r.lo; out[S - 1 - p] = r.hi;
                        }
                        Lp[2 * k1] = y1.x;
                        Lp[2 * k1 + 1] = y2.y;
                    }
                    __syncthreads();
                    if (S == BS) break;                              // ulcDecoder.c:242-245
                    // reversed-time centring FIFO in lap[M .. BS/2) (ulcDecoder.c:253-272)
                    const int avail = (BS - S) >> 1;
                    for (int q = tid; q < avail; q += WG) tmpq[q] = Lp[H2 - 1 - q];      // queue[q], q = 0 is the oldest
                    __syncthreads();
                    for (int n = tid; n < S; n += WG)
                        dst[dpos + n] = (n < avail) ? tmpq[n] : dec[n - avail];
                    if (S <= avail) {
                        for (int q = tid; q < avail; q += WG)
                            Lp[H2 - 1 - q] = (q < avail - S) ? tmpq[q + S] : dec[q - (avail - S)];
                    } else {
                        for (int q = tid; q < avail; q += WG) Lp[H2 - 1 - q] = dec[S - avail + q];
                    }
                    __syncthreads();
                    dpos += S; j++;
                } while (pat >>= 4);
                newLast = last;
                // inverse M/S + interleave once both members of a pair (or a trailing single) are staged
                const bool pairDone = LR || PART || (ch & 1) || (ch == C - 1);   // (LR, PART: every channel goes out as it stands)
                if (pairDone) {
                    __syncthreads();
                    if (warm) {
                    } else if (!LR && !PART && (ch & 1)) {
                        const float *dm = scr, *ds = scr + BS;
                        for (int n = tid; n < BS; n += WG) {
                            const float m = dm[n], sd = ds[n];                            // ulcDecoder.c:281-289
                            const float l = m + sd, r = m - sd;
                            if constexpr (SAMP) { sb.one(sb.plane(ch - 1), n, l); sb.one(sb.plane(ch), n, r); }
                            else if (C == 2) st2(outp + 2 * n, l, r);
                            else { st1(outp + (size_t)n * C + ch - 1, l); st1(outp + (size_t)n * C + ch, r); }
                        }
                    } else {
                        for (int n = tid; n < BS; n += WG) { if constexpr (SAMP) sb.one(sb.plane(PART ? ch >> 1 : ch), n, dst[n]); else st1(outp + (size_t)n * C + ch, dst[n]); }
                    }
                    __syncthreads();
                }
            }
            lastSub = newLast;
        }
        if constexpr (!PLANE) seed = rng_jump(c.jumpT, seed, (uint32_t)c.draws[blk]);      // the one RNG chain of the stream (ulcDecoder.c:75-81)
    }
    if (tid == 0) { c.lastSub[s] = lastSub; c.seed[s] = seed; c.dead[s] = dead; }
}

// ---------------------------------------------------------------------------
// Mid / side crops of stereo rows (ulcx_decode_crops_part_*; reduced BlockSize <= 4096): one workgroup = ONE wave = one row, one
// coded channel.  Where k_dsyn spends two waves, two FFT arrays and the barriers between them on a block, a row here costs one wave
// and one padded array; nothing waits for another wave.  The pieces are k_dsyn's per-wave ones - synth_unit<LOW> on the walk's
// records (SynLow's clip; lgD 0: the whole unit), the in-place pre-twiddle, fft_wave_dif / fft_wave_dif_ct, dec_time_wave for a
// decimated block - and the un-decimated epilogue for one channel by one wave: post-twiddle fused with the windowed overlap
// (lap_pair: orc_imdct's products in orc_imdct's order), the pending half rewritten in place, the stores through SampBlk, no un-mix.
// No cut: the grid is the rows, a row is entered as a range is - zero lapping state, the index's generator state, the block in front
// run without output - and its workgroup walks its blocks in order.  The state at the side channel's units is the block's state
// jumped over unitDraws[4 + j]: every draw of the mid channel lies in front of it.  The lapping state is the row's own half-row
// of the shadow state, in global memory (L2-hot: re-read by the wave that wrote it one block earlier).
// DEC_MAXT, TWL, BSC: as k_dsyn's, for the reduced geometry.
// DPART_WAVES: waves per SIMD the registers are capped for.  3 (168 registers; 0 .. 84 bytes of scratch): what the LDS of a launch
// allows at BlockSize 2048 - 13.3 KB per one-wave workgroup, 12 per CU.  4 (128 registers) spills 120 .. 212 bytes; without a cap the
// kernel takes 198 .. 257 registers, two waves per SIMD or one (profiles/part_kregs.txt).
// ---------------------------------------------------------------------------
#ifndef DPART_WAVES
#define DPART_WAVES 3
#endif
#define DPART_WG 64              // threads of a workgroup: the kernel's launch bound and, in syn_launch, its launch
template <typename OUT, int DEC_MAXT, bool TWL, int BSC>
__global__ __launch_bounds__(DPART_WG, DPART_WAVES) void k_dpart(UlcxDecCtx c, SynPart mode) {
    extern __shared__ float lds[];
    const int BS = BSC ? BSC : c.BS, H2 = BS / 2;
    constexpr int C = 2;
    const int s = blockIdx.x, ch = mode.which;
    const int lane = threadIdx.x;
    const DsynLds L = dsyn_lds(BS, 1, TWL, mode.BSw, 1);
    float2 *z = (float2 *)lds;
    float2 *twl = (float2 *)(lds + L.zFloats);
    SynWave sw;
    sw.pre = (int *)(lds + L.zFloats + L.twFloats);
    sw.seedTab = (uint32_t *)(sw.pre + 64);
    sw.lane = lane;
#ifdef ULCX_DSYN_STAMPS
    sw.stp = nullptr;
#endif
    if (TWL) for (int i = lane; i < BS / 4; i += 64) twl[i] = c.T.tw[0][i];
    bool twFull = true;
    const int M0 = BS >> 1;
    float *Lp = c.lap + ((size_t)s * C + ch) * H2;               // the pending half of this row's channel: time -1 - i at Lp[i]
    const int2 ri = c.rInfo[s];
    uint32_t seed = (uint32_t)ri.y;
    int lastSub = 0, dead = 0;
    const int rowSkip = mode.s.skip[s], rowLen = mode.s.len[s];
    for (int i = lane; i < H2; i += 64) Lp[i] = 0.0f;
    __syncthreads();
    for (int k = 1 - ri.x; k < c.K; k++) {
        const int blk = s * c.K + k;
        const int wc = c.wcScan[blk];
        if (wc == 0) dead = 1;                                       // a corrupt block ends the row (ulcDecodeTool.c:154-157)
        const bool warm = k == 0;
        const size_t oblk = (size_t)s * (c.K - 1) + (warm ? 0 : k - 1);
        const SampBlk<OUT> sb = samp_blk<OUT>(out_base<OUT>(c), mode.nOut, BS, mode.s.nSamples, s, warm ? 0 : k - 1, rowSkip, rowLen);
        OUT *sp = sb.plane(0);
        const bool sal = sb.pairs(sp);
        if (!warm && lane == 0) c.bitsOut[oblk] = dead ? 0 : c.bits[blk];
        if (dead) {
            if (!warm) for (int m = sb.mLo + lane; m < sb.mHi; m += 64) st1(sb.at(sp, m), 0.0f);
            if (lane == 0) c.bits[blk] = 0;
            continue;
        }
        const int *udraw = c.unitDraws + (size_t)blk * C * 4 + ch * 4;
        const int4 *urec = c.unitRec + (size_t)blk * C * 4 + ch * 4;
        const float4 *utail = c.unitTail + (size_t)blk * C * 4 + ch * 4;
        const uint2 *prec = c.prec + (size_t)blk * c.precStride, *nrec = c.nrec + (size_t)blk * c.nrecStride;
        const float *tmag = c.tailMag + ((size_t)blk * C * 4 + ch * 4) * c.tailStride;
        const int blkDraws = c.draws[blk];
        const int chEnd = (ch + 1 < C) ? c.unitDraws[(size_t)blk * C * 4 + (ch + 1) * 4] : blkDraws;      // draws of the block up to the end of this channel
        const BlockShape shape = block_shape(BS, wc);
        const unsigned pat0 = shape.pat;
        const bool whole = shape.whole;
        const int nsub = shape.nsub;
        if (TWL && whole != twFull) {
            // twiddle tables for this block's transform sizes: the full-size one, or those of N/2, N/4, N/8 back to back (k_dsyn)
            if (whole) for (int i = lane; i < BS / 4; i += 64) twl[i] = c.T.tw[0][i];
            else for (int i = lane; i < 7 * BS / 32; i += 64) {
                const int dd = i < BS / 8 ? 1 : i < 3 * BS / 16 ? 2 : 3;
                twl[i] = c.T.tw[dd][i - (dd == 1 ? 0 : dd == 2 ? BS / 8 : 3 * BS / 16)];
            }
            twFull = whole;
            WAVE_SYNC();
        }
        // ---- coefficients -> spectra, subblock by subblock
        {
            unsigned pat = pat0; int off = 0;
            for (int j = 0; j < nsub; j++, pat >>= 4) {
                const int d = pat & 7, S = BS >> d, M = S >> 1, Mp = FFT_PADDEDS(M, DPS);
                float2 *zj = z + FFT_PADS(off >> 1, DPS);
                sw.A = (float *)zj;
                const int dj = udraw[j], dn = (j + 1 < nsub) ? udraw[j + 1] : chEnd;
                const uint32_t unitSeed = rng_jump(c.jumpT, seed, (uint32_t)dj);
                synth_unit<true>(c, sw, S, prec, nrec, urec[j], unitSeed, dn - dj, utail[j].y, tmag + (size_t)j * c.tailStride, Mp);
                // DCT-IV pre-twiddle in place: n and M-1-n together read and write the same two complex slots
                const float2 *pre = c.T.pre[d];
#pragma unroll
                for (int n = lane; n < M / 2; n += 64) {
                    const int n2 = M - 1 - n;
                    const int pn = FFT_PADS(n, DPS), pn2 = FFT_PADS(n2, DPS);
                    const float2 a = zj[pn], b = zj[pn2];            // (X[2n], X[2n+1]), (X[S-2-2n], X[S-1-2n])
                    zj[pn]  = cmulc(make_float2(a.x, b.y), pre[n]);
                    zj[pn2] = cmulc(make_float2(b.x, a.y), pre[n2]);
                }
                if constexpr (!TWL) { if (M == 1024) fft_wave_dif_ct<1024, DPS>(zj, c.T.tw[d], lane); else fft_wave_dif(zj, M, c.T.tw[d], lane, DPS); }
                else if (M == 1024) fft_wave_dif_ct<1024, DPS>(zj, twl, lane);
                else fft_wave_dif(zj, M, twl + (d <= 1 ? 0 : d == 2 ? BS / 8 : 3 * BS / 16), lane, DPS);
                off += S;
            }
        }
        if (whole) {
            // ---- un-decimated block: post-twiddle fused with the windowed overlap (oracle/orc_fourier.c orc_imdct), one channel, no un-mix.
            //      Every pending element is read and rewritten by the same lane.
            int ov = BS;                                             // ulcDecoder.c:234-239
            if (pat0 & 8) ov >>= (wc & 7);
            if (ov > lastSub) ov = lastSub;
            const int S = BS, M = M0;
            const float2 *pre = c.T.pre[0];
            const int a = (S - ov) >> 1;
            const float *fall = c.T.winFall + ov, *rise = c.T.winRise + ov;
            const int bits = 31 - __clz(M);
#pragma unroll 4
            for (int kk = lane; kk < M / 2; kk += 64) {
                const int k1 = kk, k2 = M - 1 - kk;
                const int r1 = FFT_PADS((int)(__brev((unsigned)k1) >> (32 - bits)), DPS);
                const int r2 = FFT_PADS((int)(__brev((unsigned)k2) >> (32 - bits)), DPS);
                const float2 y1 = cmulc_post(z[r1], pre[k1]), y2 = cmulc_post(z[r2], pre[k2]);      // (Re y, -Im y)
                if (!warm) {
                    const float2 Ap = *(const float2 *)(Lp + 2 * k1);
                    const float Av[2] = { Ap.x, Ap.y }, Bv[2] = { y1.y, y2.x };
                    const int   pv[2] = { M - 1 - 2 * k1, M - 2 - 2 * k1 };
                    LapPair r[2];
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int p = pv[q];
                        const bool pass = p < a;
                        float cw = 0.0f, sn = 0.0f;
                        if (!pass) { cw = fall[p - a]; sn = rise[p - a]; }
                        r[q] = lap_pair(Av[q], Bv[q], cw, sn, pass);                                // outputs at positions p and S-1-p
                    }
                    // positions pv[1] = pv[0]-1 and S-1-pv[0], S-pv[0] are neighbours
                    sb.two(sp, sal, pv[1], r[1].lo, r[0].lo);
                    sb.two(sp, sal, S - 1 - pv[0], r[0].hi, r[1].hi);
                }
                *(float2 *)(Lp + 2 * k1) = make_float2(y1.x, y2.y);
            }
            lastSub = BS;
        } else {
            // ---- decimated block: the time domain on one timeline (dec_time_wave), the pending list in place; other lanes read what this
            //      lane's last block left in global memory: ordered by the barriers
            __syncthreads();
            const int newLast = dec_time_wave<DEC_MAXT>(c, z, Lp, wc, pat0, nsub, lastSub, lane);
            __syncthreads();
            // output = times [-BS/2, BS/2): the old pending list (time -1-i at Lp[i]), then the array
            const float *t0 = (const float *)z;
            if (!warm) {
                for (int n = 2 * lane; n < H2; n += 128) sb.two(sp, sal, n, Lp[H2 - 1 - n], Lp[H2 - 2 - n]);
                for (int n = 2 * lane; n < H2; n += 128) { const float2 m = *(const float2 *)(t0 + padf(n)); sb.two(sp, sal, H2 + n, m.x, m.y); }
            }
            __syncthreads();
            // new pending list: times [BS/2, BS) of the array
            for (int i = lane; i < H2; i += 64) Lp[H2 - 1 - i] = t0[padf(H2 + i)];
            lastSub = newLast;
        }
        __syncthreads();                                             // (one wave: the order of this block's LDS and global accesses against the next block's)
        seed = rng_jump(c.jumpT, seed, (uint32_t)blkDraws);          // the one RNG chain of the stream (ulcDecoder.c:75-81)
    }
    if (lane == 0) { c.lastSub[s] = lastSub; c.seed[s] = seed; c.dead[s] = dead; }
}

// ---------------------------------------------------------------------------
// Spectra (ulcx_decode_crops_spectra_*): the call stops where the synthesis would start its transforms - the dequantised
// coefficients of every (row, block, channel), noise included, go out as they stand in the unit arrays, channels-first:
// coef [row][channel][block][BS], a block's subblocks in coded order (ulcDecoder.c:228-231: what TransformBuffer holds).
// Behind the crop walk nothing of a block depends on another block but the generator state (a jump over the draws of the rows in
// front) and liveness (no walked row up to this one is corrupt), so the grid is one workgroup per (row, output block, channel
// pair), pair fastest, and no workgroup loops over blocks.  Row 0 of the walk, the block in front, is only ever looked at for
// those two; its records are not expanded.
//   two = 1: one wave per channel of the pair, each into its own array (BS + BS/16 floats, the FFT arrays' padding: synth_unit
//            writes through padf).  LR: a barrier, then each wave forms its own channel's m + s / m - s from both arrays.
//   two = 0: two arrays do not fit a CU's LDS (spec_lds): wave 0 dequantises the pair's channels one after the other into one
//            array and all 128 threads store it.  LR: the first channel goes out with plain stores, and behind a device-scope
//            fence and a barrier the second channel's store re-reads it (each thread the 16 bytes it stored itself) and writes both.
// Live blocks: every element stored exactly once (two = 0 with LR: the first plane twice, by the same thread).  Dead blocks: +0.0f.
// ---------------------------------------------------------------------------
struct UlcxSpecArg { float *coef; int32_t *wc; int nPairs; };
struct SpecLds { int arrFloats, nArr, listInts; };
__host__ __device__ static inline SpecLds spec_lds(int BS) {
    SpecLds l;
    l.arrFloats = BS + BS / 16;                                  // = 2 * FFT_PADDEDS(BS / 2, DPS) at DPS 4: padf's layout
    l.listInts = 64 + DSYN_PWORDS(BS);                           // per dequantising wave: prefix counts, sign-parity stream
    l.nArr = (sizeof(float) * 2 * ((size_t)l.arrFloats + l.listInts) <= (size_t)ULCX_LDS_LIMIT) ? 2 : 1;
    return l;
}
// the padded array's floats [i, i + 4), i a multiple of 4 (never across a padding gap)
__device__ __forceinline__ f32x4 spec_ld4(const float *A, int i) {
    const float2 a = *(const float2 *)(A + padf(i)), b = *(const float2 *)(A + padf(i) + 2);
    f32x4 v = { a.x, a.y, b.x, b.y };
    return v;
}
// A workgroup of the expansion kernels (k_dspec, k_ddist) and its block: spec_where() is the grid - (row, output block, channel
// pair), pair fastest - and spec_block() the part those kernels share behind it: the block's liveness and its d_bits / d_wc
// entries, the generator jump, and the expansion of a channel's units into a padded array.  A dead block ends in onDead(cell), a
// live one in onLive(cell, dequant): cell is (row, first channel of the pair, output block) as an index of [c.B][C][c.K - 1], where
// the kernel's output lies, and dequant(ch, A) channel ch of the block into the array A, run by one wave.
struct SpecWg { int s, kOut, ch0, wv, lane; bool pair, two; SpecLds L; unsigned pr; };
__device__ __forceinline__ SpecWg spec_where(const UlcxDecCtx &c, int nPairs) {
    static_assert(DPS == 4, "spec_where: a unit's offset (a multiple of 32) and four consecutive floats stay clear of the padding gaps");
    const int C = c.C, N = c.K - 1;
    const int tid = threadIdx.x;
    SpecWg w;
    w.wv = __builtin_amdgcn_readfirstlane(tid >> 6); w.lane = tid & 63;
    w.L = spec_lds(c.BS);
    w.two = w.L.nArr == 2;
    const unsigned rb = blockIdx.x / (unsigned)nPairs;
    w.pr = blockIdx.x % (unsigned)nPairs;
    w.kOut = (int)(rb % (unsigned)N); w.s = (int)(rb / (unsigned)N);
    w.ch0 = 2 * (int)w.pr;
    w.pair = w.ch0 + 1 < C;
    return w;
}
template <typename DEAD, typename LIVE>
__device__ __forceinline__ void spec_block(const UlcxDecCtx &c, const SpecWg &w, int32_t *wcOut, float *lds, DEAD &&onDead, LIVE &&onLive) {
    const int BS = c.BS, C = c.C, N = c.K - 1;
    const int tid = threadIdx.x, lane = w.lane, s = w.s, k = w.kOut + 1;
    const int blk = s * c.K + k;
    // entering the block: liveness and the draws of the walked rows in front (k_dsyn's RANGE entry; at most maxBlocksPerCall terms)
    const int2 ri = c.rInfo[s];
    int bad = 0; uint32_t dsum = 0;
    for (int j = 1 - ri.x + lane; j <= k; j += 64) {
        const int bj = s * c.K + j;
        if (c.wcScan[bj] == 0) bad = 1;
        if (j < k) dsum += (uint32_t)c.draws[bj];
    }
    const bool dead = __ballot(bad) != 0ull;                     // (each wave for itself, both the same: uniform over the workgroup)
    const size_t oblk = (size_t)s * N + w.kOut;
    const int wc = dead ? 0 : c.wcScan[blk];
    if (w.pr == 0 && tid == 0) { c.bitsOut[oblk] = dead ? 0 : c.bits[blk]; wcOut[oblk] = wc; }
    const size_t cell = ((size_t)s * C + w.ch0) * N + w.kOut;
    if (dead) { onDead(cell); return; }
    const uint32_t seed = rng_jump(c.jumpT, (uint32_t)ri.y, (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_add(dsum), 63));
    const int *udraw = c.unitDraws + (size_t)blk * C * 4;
    const int4 *urec = c.unitRec + (size_t)blk * C * 4;
    const float4 *utail = c.unitTail + (size_t)blk * C * 4;
    const uint2 *prec = c.prec + (size_t)blk * c.precStride, *nrec = c.nrec + (size_t)blk * c.nrecStride;
    const float *tmag = c.tailMag + (size_t)blk * C * 4 * c.tailStride;
    const BlockShape shape = block_shape(BS, wc);
    const int nsub = shape.nsub;
    auto unit_draws = [&](int ch, int j) { return ((j + 1 < nsub) ? udraw[ch * 4 + j + 1] : (ch + 1 < C) ? udraw[(ch + 1) * 4] : c.draws[blk]) - udraw[ch * 4 + j]; };
    SynWave sw;
    sw.pre = (int *)(lds + (size_t)w.L.nArr * w.L.arrFloats) + (w.two ? w.wv : 0) * w.L.listInts;
    sw.seedTab = (uint32_t *)(sw.pre + 64);
    sw.lane = lane;
#ifdef ULCX_DSYN_STAMPS
    sw.stp = nullptr;
#endif
    // channel ch of the block into A: its units one behind the other, each cleared behind its own record loads
    auto dequant = [&](int ch, float *A) {
        int off = 0;
        for (int j = 0; j < nsub; j++) {
            const int S = BS >> ((shape.pat >> (4 * j)) & 7), us = ch * 4 + j;
            sw.A = A + padf(off);
            const uint32_t unitSeed = rng_jump(c.jumpT, seed, (uint32_t)udraw[us]);
            synth_unit(c, sw, S, prec, nrec, urec[us], unitSeed, unit_draws(ch, j), utail[us].y, tmag + (size_t)us * c.tailStride, (S + S / 16) >> 1);
            off += S;
        }
    };
    onLive(cell, dequant);
}
template <bool LR>
__global__ __launch_bounds__(WG) void k_dspec(UlcxDecCtx c, UlcxSpecArg sp) {
    extern __shared__ float lds[];
    const int BS = c.BS, N = c.K - 1;
    const int tid = threadIdx.x;
    const SpecWg w = spec_where(c, sp.nPairs);
    const int wv = w.wv, lane = w.lane, ch0 = w.ch0;
    const bool pair = w.pair;
    const SpecLds L = w.L;
    spec_block(c, w, sp.wc, lds, [&](size_t cell) {
        float *pl0 = sp.coef + cell * BS, *pl1 = pl0 + (size_t)N * BS;                     // the pair's planes
        for (int i = 4 * tid; i < BS; i += 4 * WG) { st4(pl0 + i, 0.0f, 0.0f, 0.0f, 0.0f); if (pair) st4(pl1 + i, 0.0f, 0.0f, 0.0f, 0.0f); }
    }, [&](size_t cell, auto &dequant) {
        float *pl0 = sp.coef + cell * BS, *pl1 = pl0 + (size_t)N * BS;
        if (w.two) {
            float *A = lds + (size_t)wv * L.arrFloats;
            const bool mine = wv == 0 || pair;
            if (mine) dequant(ch0 + wv, A);
            float *pl = wv ? pl1 : pl0;
            if (LR && pair) {
                __syncthreads();
                const float *Am = lds, *As = lds + L.arrFloats;
                for (int i = 4 * lane; i < BS; i += 256) {
                    const f32x4 m = spec_ld4(Am, i), sd = spec_ld4(As, i);                   // ulcDecoder.c:281-289, on the coefficients
                    if (wv == 0) st4(pl + i, m.x + sd.x, m.y + sd.y, m.z + sd.z, m.w + sd.w);
                    else         st4(pl + i, m.x - sd.x, m.y - sd.y, m.z - sd.z, m.w - sd.w);
                }
            } else if (mine) {
                for (int i = 4 * lane; i < BS; i += 256) { const f32x4 v = spec_ld4(A, i); st4(pl + i, v.x, v.y, v.z, v.w); }
            }
        } else {
            float *A = lds;
            if (wv == 0) dequant(ch0, A);
            __syncthreads();
            for (int i = 4 * tid; i < BS; i += 4 * WG) {
                const f32x4 v = spec_ld4(A, i);
                if (LR && pair) *(f32x4 *)(pl0 + i) = v;                                      // (read again below: not non-temporal)
                else st4(pl0 + i, v.x, v.y, v.z, v.w);
            }
            if (!pair) return;
            if (LR) __threadfence();
            __syncthreads();                                                                  // the array is free again; LR: plane 0 is visible
            if (wv == 0) dequant(ch0 + 1, A);
            __syncthreads();
            for (int i = 4 * tid; i < BS; i += 4 * WG) {
                const f32x4 sd = spec_ld4(A, i);
                if (LR) {
                    const f32x4 m = *(const f32x4 *)(pl0 + i);
                    st4(pl0 + i, m.x + sd.x, m.y + sd.y, m.z + sd.z, m.w + sd.w);
                    st4(pl1 + i, m.x - sd.x, m.y - sd.y, m.z - sd.z, m.w - sd.w);
                } else st4(pl1 + i, sd.x, sd.y, sd.z, sd.w);
            }
        }
    });
}

// ---------------------------------------------------------------------------
// Distortion (ulcx_decode_crops_distortion_*): k_dspec's sibling that loads where k_dspec stores.  Behind the same entry and the
// same expansion into the padded arrays, each channel's BS coefficients y and the caller's reference plane r (16 bytes per lane,
// non-temporal; absent: +0.0f, nothing read) give per segment of W = BS / nSeg coefficients the sums S = r^2, Y = y^2,
// E = (r - y)^2, every term formed in binary64 and added by THE PAIRWISE TREE OVER ADJACENT ELEMENTS, so the result is one
// defined bit pattern (include/ulc_amd.h).  One wave per channel:
//   lane l of run q (256 coefficients) holds elements 256 q + 4 l .. + 3: (t0 + t1) + (t2 + t3), the tree's levels 1 and 2;
//   xor butterflies over 1, 2, 4, .. lanes are its levels up to a run (IEEE addition is commutative: both partners of a step
//   hold the node's bits).  W <= 256: the butterfly stops at W / 4 lanes and the first lane of each group stores.
//   W > 256: lane q & 63 keeps run q's total (runs 64 .. 127 of BlockSize 32768 in a second set), and a second butterfly over
//   the kept totals is the tree from a run up to the segment; 128 runs per segment: the two sets' totals added.
// two = 0 (BlockSize 32768, mid/side only: LR is refused by the API): wave 0 takes the pair's channels one after the other
// through the one array.  Dead blocks: +0.0 in every sum.  Every entry of the block's [channel][nSeg][3] is stored exactly once.
// ---------------------------------------------------------------------------
struct UlcxDistArg { const float *ref; int nRef, nRefBlocks; const int32_t *refRow, *refFirst; int nSeg; double *dist; int32_t *wc; int nPairs; };
struct Dist3 { double S, Y, E; };
__device__ __forceinline__ Dist3 dist_terms(const f32x4 r, const f32x4 y) {
    const double r0 = r.x, r1 = r.y, r2 = r.z, r3 = r.w, y0 = y.x, y1 = y.y, y2 = y.z, y3 = y.w;
    const double d0 = r0 - y0, d1 = r1 - y1, d2 = r2 - y2, d3 = r3 - y3;
    Dist3 t;
    t.S = (r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3);
    t.Y = (y0 * y0 + y1 * y1) + (y2 * y2 + y3 * y3);
    t.E = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    return t;
}
__device__ __forceinline__ void dist_xor(Dist3 &t, int m) { t.S += __shfl_xor(t.S, m); t.Y += __shfl_xor(t.Y, m); t.E += __shfl_xor(t.E, m); }
__device__ __forceinline__ void dist_store(double *p, const Dist3 &t) { p[0] = t.S; p[1] = t.Y; p[2] = t.E; }
// one wave, one channel: y4(i) the channel's coefficients [i, i + 4), rp its reference plane or NULL, out its [nSeg][3]
template <typename Y4>
__device__ __forceinline__ void dist_channel(int BS, int nSeg, int lane, const float *rp, double *out, Y4 &&y4) {
    const int W = BS / nSeg;
    const int group = W / 4 < 64 ? W / 4 : 64;                   // lanes of a run that share a segment
    const f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
    Dist3 k0 = { 0.0, 0.0, 0.0 }, k1 = { 0.0, 0.0, 0.0 };
    f32x4 rn = rp ? __builtin_nontemporal_load((const f32x4 *)(rp + 4 * lane)) : zero;
    for (int i = 4 * lane, q = 0; i < BS; i += 256, q++) {
        const f32x4 r = rn;
        if (rp && i + 256 < BS) rn = __builtin_nontemporal_load((const f32x4 *)(rp + i + 256));
        Dist3 t = dist_terms(r, y4(i));
        for (int m = 1; m < group; m <<= 1) dist_xor(t, m);
        if (W <= 256) { if (!(lane & (group - 1))) dist_store(out + 3 * (size_t)(i / W), t); }
        else if (lane == (q & 63)) { if (q < 64) k0 = t; else k1 = t; }
    }
    if (W <= 256) return;
    const int runs = W / 256, R = BS / 256;                      // runs per segment (2 .. 128), runs of the block
    const int span = runs < 64 ? runs : 64;
    for (int m = 1; m < span; m <<= 1) { dist_xor(k0, m); if (R > 64) dist_xor(k1, m); }
    if (runs == 128) {
        if (lane == 0) { const Dist3 t = { k0.S + k1.S, k0.Y + k1.Y, k0.E + k1.E }; dist_store(out, t); }
    } else if (lane < (R < 64 ? R : 64) && !(lane & (span - 1))) {
        dist_store(out + 3 * (size_t)(lane / runs), k0);
        if (R > 64) dist_store(out + 3 * (size_t)((64 + lane) / runs), k1);
    }
}
template <bool LR>
__global__ __launch_bounds__(WG) void k_ddist(UlcxDecCtx c, UlcxDistArg da) {
    extern __shared__ float lds[];
    const int BS = c.BS, N = c.K - 1, nSeg = da.nSeg;
    const int tid = threadIdx.x;
    const SpecWg w = spec_where(c, da.nPairs);
    const int wv = w.wv, lane = w.lane, ch0 = w.ch0;
    const bool pair = w.pair;
    const SpecLds L = w.L;
    const size_t och = (size_t)N * nSeg * 3, rch = (size_t)da.nRefBlocks * BS;             // from a channel to the next one: sums, reference
    spec_block(c, w, da.wc, lds, [&](size_t cell) {
        double *o0 = da.dist + cell * nSeg * 3;                                            // the pair's sums: these and the ones och behind
        for (int i = tid; i < 3 * nSeg; i += WG) { o0[i] = 0.0; if (pair) o0[och + i] = 0.0; }
    }, [&](size_t cell, auto &dequant) {
        double *o0 = da.dist + cell * nSeg * 3;
        // the block's reference planes: absent without d_ref, for a row or a block outside the reference (the index in 64 bits)
        const float *rp = nullptr;
        if (da.ref) {
            const int row = da.refRow ? da.refRow[w.s] : w.s;
            const long long rb = (long long)(da.refFirst ? da.refFirst[w.s] : 0) + w.kOut;
            if (row >= 0 && row < da.nRef && rb >= 0 && rb < da.nRefBlocks) rp = da.ref + (((size_t)row * c.C + ch0) * da.nRefBlocks + (size_t)rb) * BS;
        }
        if (w.two) {
            float *A = lds + (size_t)wv * L.arrFloats;
            const bool mine = wv == 0 || pair;
            if (mine) dequant(ch0 + wv, A);
            const float *rw = rp ? rp + wv * rch : nullptr;
            if (LR && pair) {
                __syncthreads();
                const float *Am = lds, *As = lds + L.arrFloats;
                dist_channel(BS, nSeg, lane, rw, o0 + wv * och, [&](int i) {
                    const f32x4 m = spec_ld4(Am, i), sd = spec_ld4(As, i);                   // what k_dspec<true> stores
                    const f32x4 l = { m.x + sd.x, m.y + sd.y, m.z + sd.z, m.w + sd.w }, r = { m.x - sd.x, m.y - sd.y, m.z - sd.z, m.w - sd.w };
                    return wv == 0 ? l : r;
                });
            } else if (mine) dist_channel(BS, nSeg, lane, rw, o0 + wv * och, [&](int i) { return spec_ld4(A, i); });
        } else if (wv == 0) {
            float *A = lds;
            for (int h = 0; h < (pair ? 2 : 1); h++) {
                dequant(ch0 + h, A);
                dist_channel(BS, nSeg, lane, rp ? rp + h * rch : nullptr, o0 + h * och, [&](int i) { return spec_ld4(A, i); });
            }
        }
    });
}
size_t ulcx_spec_lds_bytes(int BS) {
    const SpecLds l = spec_lds(BS);
    return sizeof(float) * (size_t)l.nArr * ((size_t)l.arrFloats + l.listInts);
}
int ulcx_spec_arrays(int BS) { return spec_lds(BS).nArr; }

size_t ulcx_dec_lds_bytes(int BS, int fast, int twInLds, int listBS, int oneWave) {
    DsynLds l = dsyn_lds(BS, fast, twInLds, listBS, oneWave);
    return sizeof(float) * ((size_t)l.zFloats + l.twFloats + l.listFloats);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ulcx_set_error("%s: %s", #x, hipGetErrorString(e_)); return ULCX_ERR_HIP; } } while (0)

// The synthesis instantiation of a context in a mode, THE one place that maps a geometry to its kernel: what is launched, what has its
// dynamic-LDS limit raised and what is asked for its occupancy are this pointer, typed by the mode it takes.  (fastOK means stereo up to BlockSize
// 4096: with DSYN_C4096 the run-time BlockSize kernel of 32 trips does not exist.  A cut of a plain call is k_dsyn's alone: no k_dgen<SynCut> either.)
template <typename OUT, typename MODE> using SynFn = void (*)(UlcxDecCtx, MODE);
template <typename OUT, typename MODE> static SynFn<OUT, MODE> syn_pick(const UlcxDecCtx &cc) {
    constexpr bool TW = DSYN_TWL != 0;
    if constexpr (MODE::part) {                                     // stereo up to BlockSize 4096: one wave per row (k_dpart)
        if (!cc.fastOK) return k_dgen<OUT, MODE>;
        if (cc.BS == 2048) return k_dpart<OUT, 16, TW, 2048>;
        if (cc.BS < 2048) return k_dpart<OUT, 16, TW, 0>;
        return k_dpart<OUT, 32, false, 4096>;
    } else {
    if (!cc.fastOK) { if constexpr (MODE::split && !MODE::range) return nullptr; else return k_dgen<OUT, MODE>; }
    if (cc.BS == 2048 && DSYN_C2048) return k_dsyn<OUT, 16, TW, 2048, MODE>;
    if (cc.BS <= 2048) return k_dsyn<OUT, 16, TW, 0, MODE>;
    if constexpr (DSYN_C4096) return k_dsyn<OUT, 32, false, 4096, MODE>;
    else return k_dsyn<OUT, 32, false, 0, MODE>;
    }
}
// a synthesis kind as its mode type: f(MODE{})
template <typename F> static auto syn_with_mode(UlcxSynKind kind, F &&f) {
    switch (kind) {
    case ULCX_SYN_CUT:       return f(SynCut{});
    case ULCX_SYN_RANGE:     return f(SynRange{});
    case ULCX_SYN_SAMPLES:   return f(SynSamples{});
    case ULCX_SYN_PLANES:    return f(SynPlanes<false>{});
    case ULCX_SYN_PLANES_LR: return f(SynPlanes<true>{});
    case ULCX_SYN_LOW:       return f(SynLow{});
    case ULCX_SYN_PART:      return f(SynPart{});
    default:                 return f(SynWhole{});
    }
}
// A launch with more than 48 KiB of dynamic LDS: raise the kernel's limit to this launch's size (ulcx_enc.hip: allow_lds).
static hipError_t allow_lds(const void *fn, size_t lds) {
    return lds > 48 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

template <typename OUT> static const void *syn_fn(const UlcxDecCtx &cc, UlcxSynKind kind) {       // (ULCX_SYN_LOW: cc the context of the REDUCED geometry)
    return syn_with_mode(kind, [&](auto m) { return (const void *)syn_pick<OUT, decltype(m)>(cc); });
}
// resident workgroups of the stereo synthesis kernel this context runs in a mode: what an even cut of the batch is sized for
// (ULCX_SYN_LOW: c the context of the reduced geometry, walkBS the walk's BlockSize)
int ulcx_dec_syn_slots(const UlcxDecCtx &c, UlcxSynKind kind, int walkBS) {
    if (!c.fastOK) return 0;
    // what a cut would launch: the float and the PCM16 instantiation are both asked, the smaller residency sizes the cut
    const void *fns[2] = { syn_fn<float>(c, kind), syn_fn<int16_t>(c, kind) };
    const size_t lds = ulcx_dec_lds_bytes(c.BS, c.fastOK, c.twInLds, walkBS);
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    for (const void *fn : fns) {
        int p1 = 0;
        if (allow_lds(fn, lds) != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&p1, fn, WG, lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
        per = (fn == fns[0] || p1 < per) ? p1 : per;
    }
    return cus * per;
}

// A mode's fields from the call's aux data (walkBS: the BlockSize the walk ran at) and the launch of the instantiation that mode
// picks for the context: the argument is built as the type the kernel takes.
template <typename OUT, typename MODE>
static int syn_launch(const UlcxDecCtx &cs, const UlcxDecAux &aux, int walkBS, unsigned grid, size_t lds, hipStream_t st) {
    MODE m = {};
    if constexpr (MODE::samp) m.s = UlcxSampArg{ aux.samp.skip, aux.samp.lenC, aux.samp.nSamples };
    if constexpr (MODE::plane) { m.coef = aux.syn.coef; m.nPl = aux.syn.planes; }
    if constexpr (MODE::low) m.BSw = walkBS;
    if constexpr (MODE::part) { m.which = aux.part.which; m.nOut = aux.part.planes; }
    const SynFn<OUT, MODE> fn = syn_pick<OUT, MODE>(cs);
    if (!fn) { ulcx_set_error("synthesis: no kernel of this mode for %d channels of BlockSize %d", cs.C, cs.BS); return ULCX_ERR_ARG; }
    CK(allow_lds((const void *)fn, lds));
    unsigned threads = WG;                                       // by the kernel that was picked: every instantiation of k_dpart is one wave
    if constexpr (MODE::part) { if (fn != k_dgen<OUT, MODE>) threads = DPART_WG; }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, st, cs, m);
    return ULCX_OK;
}
// Two kernels on the caller's stream: the syntax walk, then the synthesis.  (Measured and dropped, profiles/NOTES_r01-r04.md:
// the walk of a chunk of streams / of the second half of the blocks beside the synthesis of the previous one - the
// synthesis slows down by more than the walk it hides.)  What the two are follows from aux.kind alone.
int ulcx_dec_launch(const UlcxDecCtx &cIn, hipStream_t st, hipEvent_t *ev, const UlcxDecAux &aux) {
    int stage = 0;
    if (ev) CK(hipEventRecord(ev[stage++], st));
    const UlcxDecKind kind = aux.kind; const bool range = kind != ULCX_DEC_PLAIN, part = kind == ULCX_DEC_PART, low = kind == ULCX_DEC_LOWRATE || part;
    UlcxDecCtx c = cIn;
    c.s0 = 0; c.s1 = c.B; c.k0 = range ? 1 : 0; c.k1 = c.K;
    // a low-rate call: the walk runs on c, the file's geometry; the rows and the synthesis on cs, the context of BlockSize >> lgD -
    // its tables, its kernel pick and its lapping scratch - which still addresses the walk's per-block rows and records
    UlcxDecCtx cs = c;
    if (low) {
        cs.BS = c.BS >> aux.low.lgD; cs.lgBS = c.lgBS - aux.low.lgD; cs.T = aux.low.T; cs.fastOK = aux.low.fast; cs.twInLds = aux.low.twInLds;
        cs.lapScratch = aux.low.lapScratch;
    }
    // the rows (sample crops: from (start, len); a synth call: from the window codes, in place of every walk), then the walk: indexed over a
    // crop call's corpus or, for a range call, over the decoder's own streams as a strided corpus (file = stream)
    if (kind == ULCX_DEC_SYNTH) hipLaunchKernelGGL(k_synth_rows, dim3((unsigned)(((long long)c.B * c.K + 63) / 64)), dim3(64), 0, st, c.B, c.K, aux.syn.planes, aux.syn.wc,
                                                   c.wcScan, c.draws, c.bits, c.rInfo, aux.samp.skip, aux.samp.lenC, aux.samp.nSamples);
    else {
    if (kind == ULCX_DEC_SAMPLES || low) hipLaunchKernelGGL(k_crop_sample_rows, dim3((c.B + 63) / 64), dim3(64), 0, st, c.B, cs.BS, aux.samp.nSamples, aux.samp.start,
                                                            aux.samp.len, aux.samp.first, aux.samp.count, aux.samp.skip, aux.samp.lenC);
    if (ulcx_dec_has_corpus(kind)) hipLaunchKernelGGL(k_dscan_rows, dim3((c.B * c.K + 63) / 64), dim3(64), 0, st, c, aux.corpus, aux.cropFile, aux.cropCount);
    else if (kind == ULCX_DEC_RANGE) hipLaunchKernelGGL(k_dscan_rows, dim3((c.B * c.K + 63) / 64), dim3(64), 0, st, c,
                                         ulcx_corpus_strided(c.B, c.in, c.payStride, c.payBytes, c.rIndex, c.rIndexStride, c.rIndexBlocks), nullptr, nullptr);
    else if (c.packed) hipLaunchKernelGGL(k_dscan_packed, dim3((c.B + 63) / 64), dim3(64), 0, st, c);
    else hipLaunchKernelGGL(k_dscan, dim3((c.B * c.K + 63) / 64), dim3(64), 0, st, c);
    }
    if (ev) CK(hipEventRecord(ev[stage++], st));
    if (!ulcx_dec_has_synthesis(kind)) {
        const bool dist = kind == ULCX_DEC_DISTORTION;
        const void *fn = dist ? (aux.spec.lr ? (const void *)k_ddist<true> : (const void *)k_ddist<false>)
                              : (aux.spec.lr ? (const void *)k_dspec<true> : (const void *)k_dspec<false>);
        const size_t slds = ulcx_spec_lds_bytes(c.BS);
        const int nPairs = (c.C + 1) / 2;
        const long long g = (long long)c.B * (c.K - 1) * nPairs;
        if (g > 0x7FFFFFFFLL) { ulcx_set_error("%s call: %lld workgroups", dist ? "distortion" : "spectra", g); return ULCX_ERR_ARG; }
        CK(allow_lds(fn, slds));
        UlcxSpecArg sp = { aux.spec.coef, aux.spec.wc, nPairs };
        UlcxDistArg da = { aux.dist.ref, aux.dist.nRef, aux.dist.refBlocks, aux.dist.refRow, aux.dist.refFirst, aux.dist.seg, aux.dist.out, aux.spec.wc, nPairs };
        void *args[] = { &c, dist ? (void *)&da : (void *)&sp };
        CK(hipLaunchKernel(fn, dim3((unsigned)g), dim3(WG), args, slds, st));
    } else if (!(ULCX_DBG(c) & 8)) {
        const bool split = cs.fastOK && aux.synGrid > 0 && !part;
        const UlcxSynKind syn = part ? ULCX_SYN_PART : low ? ULCX_SYN_LOW : kind == ULCX_DEC_SYNTH ? (aux.syn.lr ? ULCX_SYN_PLANES_LR : ULCX_SYN_PLANES)
                              : kind == ULCX_DEC_SAMPLES ? ULCX_SYN_SAMPLES : range ? ULCX_SYN_RANGE : split ? ULCX_SYN_CUT : ULCX_SYN_WHOLE;
        const size_t lds = ulcx_dec_lds_bytes(cs.BS, cs.fastOK, cs.twInLds, low ? c.BS : 0, part ? 1 : 0);
        const unsigned g = split ? (unsigned)aux.synGrid : (unsigned)c.B;
        cs.synFull = split ? aux.synFull : (range && cs.fastOK) ? c.B : 0;        // (a range call without a cut: every workgroup one whole stream)
        const int rc = syn_with_mode(syn, [&](auto m) {
            return c.pcm16 ? syn_launch<int16_t, decltype(m)>(cs, aux, c.BS, g, lds, st) : syn_launch<float, decltype(m)>(cs, aux, c.BS, g, lds, st);
        });
        if (rc) return rc;
    }
    if (ev) CK(hipEventRecord(ev[stage++], st));
    CK(hipGetLastError());
    return ULCX_OK;
}

int ulcx_index_launch(const UlcxDecCtx &c, int maxBlocks, ulcx_index_entry *d_index, int32_t *d_nBlocks, hipStream_t st) {
    hipLaunchKernelGGL(k_dindex, dim3((c.B + 63) / 64), dim3(64), 0, st, c, maxBlocks, d_index, d_nBlocks);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_index_ragged_launch(const UlcxDecCtx &c, const int64_t *d_payOffs, const int64_t *d_idxOffs, long long idxTotal, ulcx_index_entry *d_index,
                             int32_t *d_nBlocks, hipStream_t st) {
    hipLaunchKernelGGL(k_dindex_ragged, dim3((c.B + 63) / 64), dim3(64), 0, st, c, d_payOffs, d_idxOffs, idxTotal, d_index, d_nBlocks);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_index_begin_launch(int nRows, ulcx_index_entry *d_index, int indexStride, int32_t *d_nBlocks, hipStream_t st) {
    const long long nEnt = (long long)nRows * indexStride;
    hipLaunchKernelGGL(k_dindex_begin, dim3((unsigned)((nEnt + 255) / 256)), dim3(256), 0, st, nEnt, indexStride, d_index, d_nBlocks);
    CK(hipGetLastError());
    return ULCX_OK;
}
// c.in / c.slot / c.inBytes: the slots, as for a slot-form decode call of nRows streams
int ulcx_index_slots_launch(const UlcxDecCtx &c, int nRows, int nBlocks, const int32_t *d_bits, ulcx_index_entry *d_index, int indexStride,
                            int32_t *d_nBlocks, hipStream_t st) {
    const long long nAll = (long long)nRows * nBlocks;
    hipLaunchKernelGGL(k_dindex_slots_walk, dim3((unsigned)((nAll + 63) / 64)), dim3(64), 0, st, c, nAll, nBlocks, d_bits, d_index, indexStride, d_nBlocks);
    hipLaunchKernelGGL(k_dindex_slots_scan, dim3(nRows), dim3(64), 0, st, c.jumpT, nBlocks, d_index, indexStride, d_nBlocks);
    CK(hipGetLastError());
    return ULCX_OK;
}

// c.in / c.inBytes: the source's whole payload buffer, as a.src has it; geometry and tables are all else that is read of c
int ulcx_splice_launch(const UlcxDecCtx &c, const UlcxSpliceArgs &a, hipStream_t st) {
    const long long nEnt = (long long)a.nOut * a.outIndexStride, nBlk = (long long)a.nOut * (a.outIndexStride - 1);
    // aligned 16-byte lines a file of outPayStride bytes can touch, wherever it starts
    const long long lines = (a.outPayStride + 15 + 15) / 16, nLines = (long long)a.nOut * lines;
    hipLaunchKernelGGL(k_dindex_begin, dim3((unsigned)((nEnt + 255) / 256)), dim3(256), 0, st, nEnt, a.outIndexStride, a.outIndex, a.outIndexBlocks);
    hipLaunchKernelGGL(k_splice_plan, dim3(a.nOut), dim3(64), 0, st, a.nSeg, a.segOffs, a.seg, a.segStart);
    const bool ragged = a.src.payOffs != nullptr;
    hipLaunchKernelGGL(ragged ? k_splice_walk<true> : k_splice_walk<false>, dim3((unsigned)((nBlk + 63) / 64)), dim3(64), 0, st, c, a.src, nBlk, a.nSeg, a.segOffs, a.seg,
                       a.segStart, a.outIndex, a.outIndexStride);
    hipLaunchKernelGGL(k_splice_scan, dim3(a.nOut), dim3(64), 0, st, c.jumpT, a.outIndex, a.outIndexStride, a.outPayStride, a.outPayBytes, a.outMaxBlock, a.outIndexBlocks);
    hipLaunchKernelGGL(ragged ? k_splice_copy<true> : k_splice_copy<false>, dim3((unsigned)((nLines + SPLICE_COPY_WG - 1) / SPLICE_COPY_WG)), dim3(SPLICE_COPY_WG), 0, st,
                       a.src, nLines, lines, a.nSeg, a.segOffs, a.seg, a.segStart, a.outIndex, a.outIndexStride, a.outIndexBlocks, a.outPay, a.outPayStride);
    CK(hipGetLastError());
    return ULCX_OK;
}

// ---------------------------------------------------------------------------
// Slots -> contiguous per-stream payloads (tools/ulcEncodeTool.c:160-169)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_streams(int nBlocks, int slotBytes, const uint8_t *slots, const int32_t *bits,
                                                       uint8_t *payload, long long stride, int32_t *payloadBytes, int32_t *maxBlock) {
    int s = blockIdx.x, tid = threadIdx.x;
    uint8_t *dst = payload + (size_t)s * stride;
    int off = 0, mx = 0;
    for (int k = 0; k < nBlocks; k++) {
        int n = (bits[(size_t)s * nBlocks + k] + 7) >> 3;
        const uint8_t *src = slots + ((size_t)s * nBlocks + k) * slotBytes;
        if ((size_t)off + n <= (size_t)stride) for (int i = tid; i < n; i += 256) dst[off + i] = src[i];
        off += n;
        mx = n > mx ? n : mx;
    }
    if (tid == 0) { payloadBytes[s] = off; if (maxBlock) maxBlock[s] = mx; }
}
int ulcx_pack_launch(int nStreams, int nBlocks, int slotBytes, const uint8_t *d_slots, const int32_t *d_bits, uint8_t *d_payload,
                     long long stride, int32_t *d_payloadBytes, int32_t *d_maxBlock, hipStream_t st) {
    hipLaunchKernelGGL(k_pack_streams, dim3(nStreams), dim3(256), 0, st, nBlocks, slotBytes, d_slots, d_bits, d_payload, stride, d_payloadBytes, d_maxBlock);
    CK(hipGetLastError());
    return ULCX_OK;
}
