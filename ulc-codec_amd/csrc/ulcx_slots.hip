// ulcx_slots.hip — stream slots (include/ulc_amd.h, "Stream slots"): copies of single streams' persistent state between an
// object's arrays and a set of rows - the compact shadow state a subset call launches on, or the caller's saved records.
//
// A stream's state is one large row (encoder: hist [2*BS][C]; decoder: lap [C][BS/2]; both multiples of 16 bytes for every
// accepted geometry) and a few words (encoder: one UlcxWcState; decoder: lastSub, seed, dead, packOff).  Both sides of a copy
// are described by the same UlcxSlotRows (base pointers and byte strides), so gather, scatter, save and load are two kernels:
//   k_slots_gather    rows[i]        <- object[slots[i]]   (an entry outside [0, B): the state right after create)
//   k_slots_scatter   object[slots[i]] <- rows[i]          (an entry outside [0, B), or a record whose header differs: skipped)
//   k_slots_reset     object[slots[i]] <- the state right after create
// One workgroup per listed slot (a grid-stride share above ULCX_SLOTS_GRID), 16-byte loads and stores on the large row.
// Plain C++ vector accesses only.
#include "ulcx_internal.h"

#define SLOTS_WG 256
#define ULCX_SLOTS_GRID 16384

// word w of small array a in the state right after create (enc_reset_state / dec_reset_state, ulcx_api.cpp)
__device__ static inline uint32_t slots_fresh_word(int isEnc, int a, int w) {
    if (isEnc) return (w == (int)(offsetof(UlcxWcState, wcPrev) / 4) || w == (int)(offsetof(UlcxWcState, wcCur) / 4)) ? 0x10u : 0u;
    return a == 1 ? 1234567u : 0u;                             // decoder: {lastSub, seed, dead, packOff}
}
__device__ static inline uint4 *slots_big(const UlcxSlotRows &r, size_t row) { return (uint4 *)(r.big + row * r.bigStride); }
__device__ static inline uint32_t *slots_small(const UlcxSlotRows &r, int a, size_t row) { return (uint32_t *)(r.small[a] + row * r.smallStride); }

__global__ __launch_bounds__(SLOTS_WG) void k_slots_gather(UlcxSlotRows obj, UlcxSlotRows rows, const int32_t *slots, int n, UlcxSlotGeom g) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int s = slots[i];
        const bool ok = (unsigned)s < (unsigned)g.B;
        uint4 *dst = slots_big(rows, (size_t)i);
        if (ok) {
            const uint4 *src = slots_big(obj, (size_t)s);
            for (int v = threadIdx.x; v < g.rowVec; v += SLOTS_WG) dst[v] = src[v];
        } else {
            for (int v = threadIdx.x; v < g.rowVec; v += SLOTS_WG) dst[v] = make_uint4(0u, 0u, 0u, 0u);
        }
        // the words; a record pads them to a multiple of 16 bytes (padWords >= smallWords, zeros behind the state)
        for (int t = threadIdx.x; t < g.nSmall * g.padWords; t += SLOTS_WG) {
            const int a = t / g.padWords, w = t % g.padWords;
            uint32_t x = 0u;
            if (w < g.smallWords) x = ok ? slots_small(obj, a, (size_t)s)[w] : slots_fresh_word(g.isEnc, a, w);
            slots_small(rows, a, (size_t)i)[w] = x;
        }
        if (rows.hdr && threadIdx.x == 0) *(uint4 *)(rows.hdr + (size_t)i * rows.hdrStride) = g.header;
    }
}

__global__ __launch_bounds__(SLOTS_WG) void k_slots_scatter(UlcxSlotRows obj, UlcxSlotRows rows, const int32_t *slots, int n, UlcxSlotGeom g) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int s = slots[i];
        if ((unsigned)s >= (unsigned)g.B) continue;                      // (uniform over the workgroup)
        if (rows.hdr) {                                                  // a record of another kind / geometry / rate: the slot stays as it was
            const uint4 h = *(const uint4 *)(rows.hdr + (size_t)i * rows.hdrStride);
            if (h.x != g.header.x || h.y != g.header.y || h.z != g.header.z || h.w != g.header.w) continue;
        }
        const uint4 *src = slots_big(rows, (size_t)i);
        uint4 *dst = slots_big(obj, (size_t)s);
        for (int v = threadIdx.x; v < g.rowVec; v += SLOTS_WG) dst[v] = src[v];
        for (int t = threadIdx.x; t < g.nSmall * g.smallWords; t += SLOTS_WG) {
            const int a = t / g.smallWords, w = t % g.smallWords;
            slots_small(obj, a, (size_t)s)[w] = slots_small(rows, a, (size_t)i)[w];
        }
    }
}

__global__ __launch_bounds__(SLOTS_WG) void k_slots_reset(UlcxSlotRows obj, const int32_t *slots, int n, UlcxSlotGeom g) {
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int s = slots[i];
        if ((unsigned)s >= (unsigned)g.B) continue;
        uint4 *dst = slots_big(obj, (size_t)s);
        for (int v = threadIdx.x; v < g.rowVec; v += SLOTS_WG) dst[v] = make_uint4(0u, 0u, 0u, 0u);
        for (int t = threadIdx.x; t < g.nSmall * g.smallWords; t += SLOTS_WG) {
            const int a = t / g.smallWords, w = t % g.smallWords;
            slots_small(obj, a, (size_t)s)[w] = slots_fresh_word(g.isEnc, a, w);
        }
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { ulcx_set_error("%s: %s", #x, hipGetErrorString(e_)); return ULCX_ERR_HIP; } } while (0)
static unsigned slots_grid(int n) { return (unsigned)(n < ULCX_SLOTS_GRID ? n : ULCX_SLOTS_GRID); }

int ulcx_slots_gather(const UlcxSlotRows &obj, const UlcxSlotRows &rows, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st) {
    hipLaunchKernelGGL(k_slots_gather, dim3(slots_grid(n)), dim3(SLOTS_WG), 0, st, obj, rows, d_slots, n, g);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_slots_scatter(const UlcxSlotRows &obj, const UlcxSlotRows &rows, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st) {
    hipLaunchKernelGGL(k_slots_scatter, dim3(slots_grid(n)), dim3(SLOTS_WG), 0, st, obj, rows, d_slots, n, g);
    CK(hipGetLastError());
    return ULCX_OK;
}
int ulcx_slots_reset(const UlcxSlotRows &obj, const int32_t *d_slots, int n, const UlcxSlotGeom &g, hipStream_t st) {
    hipLaunchKernelGGL(k_slots_reset, dim3(slots_grid(n)), dim3(SLOTS_WG), 0, st, obj, d_slots, n, g);
    CK(hipGetLastError());
    return ULCX_OK;
}
