// ensemble.hip — geometric self-ensemble inference (the reference's test_x8, F_model_depthCond.py:236-270): the eight
// flip / transpose members of an NHWC image on the way in, their inverse maps, the output clamp and the mean on the way out.
//
//   dasr_ensemble_expand_f32   float [N,H,W,C] -> out_a [4N,H,W,C] (members 0..3) and out_t [4N,W,H,C] (members 4..7)
//   dasr_ensemble_expand_u8    the same move with 1-byte elements (the region bytes)
//   dasr_ensemble_ingest_u8    uint8 camera frames -> the eight float members: dasr_frame_ingest_u8 (x / 255, IEEE division,
//                              B <-> R with swap_rb) followed by dasr_ensemble_expand_f32, in one pass
//   dasr_ensemble_merge        y_a [4N,H,W,C], y_t [4N,W,H,C] (before the output clamp) -> out [N,H,W,C]: every member
//                              mapped back and clamped, seven additions in member order, times 0.125
//
// Member m = v + 2 h + 4 t: v flips along W, h along H, t transposes last.  Member m of image n is image (m % 4) * N + n of
// its group's tensor.  With fh(r) = h ? H-1-r : r and fv(c) = v ? W-1-c : c
//   t = 0:  x_m[n, r, c, :] = x[n, fh(r), fv(c), :]            t = 1:  x_m[n, r, c, :] = x[n, fh(c), fv(r), :]   (r < W, c < H)
// so source pixel (y, x) lands at (fh(y), fv(x)) of an A member and at (fv(x), fh(y)) of a T member.
//
// One workgroup = one 32 x 32 pixel tile (C interleaved channels per pixel) of one image.  expand / ingest: the source tile
// goes through LDS once, loaded along source rows, and all eight members are written from it along OUTPUT rows - for the
// T members an output row is a source column, read out of LDS across its rows.  merge: the four A tiles of an output tile
// are read in place (a flip only reverses a row), the four T tiles pass through LDS one after the other, the eight values
// of an element meet in a register and the tile is written once.  Row pitch in LDS: 33 C dwords for fp32 (33 C mod 32 = C:
// the lanes of a transposed access step C banks per pixel, and their C channels fill the gap), 32 C + 4 bytes for uint8 (an
// odd number of dwords, and room for the three bytes a row's misalignment shifts it by).  uint8 rows start at any byte
// address (H*W*C need not be a multiple of 4): a row is staged and stored as aligned dwords between single head and tail
// bytes.  Plain HIP, 64-bit element indices, no atomics, no inline assembly, no workspace.
#include "dasr_common.h"

#if DASR_DEVICE_BUILD
__device__ __forceinline__ float ens_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float ens_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float ens_mul(float a, float b) { return __fmul_rn(a, b); }
#else
static inline float ens_div(float a, float b) { volatile float r = a / b; return r; }
static inline float ens_add(float a, float b) { volatile float r = a + b; return r; }
static inline float ens_mul(float a, float b) { volatile float r = a * b; return r; }
#endif

#define ENS_T 32                        // tile side in pixels

template <class T, int C> struct ens_lds;
template <int C> struct ens_lds<float, C> { static constexpr int pitch = 33 * C; };                  // in elements
template <int C> struct ens_lds<unsigned char, C> { static constexpr int pitch = ENS_T * C + 4; };

// One row of n elements from g into the LDS row l.  fp32: element i at l[i].  uint8: byte i at l[((uintptr_t)g & 3) + i], so
// that aligned dwords of the source are aligned dwords of the row (l is 4-byte aligned).
__device__ __forceinline__ void ens_stage_row(const float* __restrict__ g, float* l, int n, int lane, int nlanes) {
    for (int i = lane; i < n; i += nlanes) l[i] = g[i];
}
__device__ __forceinline__ void ens_stage_row(const unsigned char* __restrict__ g, unsigned char* l, int n, int lane,
                                              int nlanes) {
    const int mis = (int)((uintptr_t)g & 3);
    int head = (4 - mis) & 3;
    if (head > n) head = n;
    const int body = (n - head) >> 2, tail = n - head - 4 * body;
    const unsigned* gs = (const unsigned*)(g + head);
    unsigned* ld = (unsigned*)(l + mis + head);
    for (int i = lane; i < body; i += nlanes) ld[i] = gs[i];
    for (int i = lane; i < head + tail; i += nlanes) {
        const int e = i < head ? i : head + 4 * body + (i - head);
        l[mis + e] = g[e];
    }
}

// Slots of an output row of at most ENS_T * C elements: a thread takes slot q of a row and writes what the slot covers.
// fp32: one element per slot.  uint8: the aligned dword q of the row's address range - one dword store when the row covers
// all of it, single bytes at the row's two ends.  val(k) is element k of the row.
template <int C> __device__ __forceinline__ constexpr int ens_slots(const float*) { return ENS_T * C; }
template <int C> __device__ __forceinline__ constexpr int ens_slots(const unsigned char*) { return (ENS_T * C + 3) / 4 + 1; }

template <class F>
__device__ __forceinline__ void ens_store_slot(float* g, int n, int q, F val) {
    if (q < n) g[q] = val(q);
}
template <class F>
__device__ __forceinline__ void ens_store_slot(unsigned char* g, int n, int q, F val) {
    const int k0 = 4 * q - (int)((uintptr_t)g & 3);               // the row element at the slot's first byte
    if (k0 >= n) return;
    if (k0 >= 0 && k0 + 4 <= n) {
        const unsigned w = (unsigned)val(k0) | ((unsigned)val(k0 + 1) << 8) | ((unsigned)val(k0 + 2) << 16) |
                           ((unsigned)val(k0 + 3) << 24);
        *(unsigned*)(g + k0) = w;
    } else {
        for (int k = k0 < 0 ? 0 : k0; k < k0 + 4 && k < n; ++k) g[k] = val(k);
    }
}

__device__ __forceinline__ float ens_convert(float v, const float*) { return v; }
__device__ __forceinline__ unsigned char ens_convert(unsigned char v, const unsigned char*) { return v; }
__device__ __forceinline__ float ens_convert(unsigned char v, const float*) { return ens_div((float)v, 255.0f); }

// ---- expand / ingest ----------------------------------------------------------------------------------------------------
// TS -> TD: float -> float and uint8 -> uint8 move, uint8 -> float divides by 255.  SWAP: output channel c is source channel
// 2 - c (C == 3).
template <class TS, class TD, int C, bool SWAP>
__global__ void __launch_bounds__(256) k_ens_expand(const TS* __restrict__ src, TD* __restrict__ out_a, TD* __restrict__ out_t,
                                                    int N, int H, int W) {
    constexpr int P = ens_lds<TS, C>::pitch;
    __shared__ __attribute__((aligned(16))) TS s_t[ENS_T * P];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * ENS_T, x0 = blockIdx.x * ENS_T;
    const int nr = H - y0 < ENS_T ? H - y0 : ENS_T, nc = W - x0 < ENS_T ? W - x0 : ENS_T;
    const size_t rowlen = (size_t)W * C;
    const TS* tile = src + ((size_t)n * H + y0) * rowlen + (size_t)x0 * C;
    for (int r = tid >> 6; r < nr; r += 4) ens_stage_row(tile + (size_t)r * rowlen, s_t + r * P, nc * C, tid & 63, 64);
    __syncthreads();
    // where row i of the tile starts inside its LDS row (uint8: the misalignment of its global address)
    const int mis0 = sizeof(TS) == 1 ? (int)((uintptr_t)tile & 3) : 0, misr = sizeof(TS) == 1 ? (int)(rowlen & 3) : 0;
    constexpr int SLOTS = ens_slots<C>((const TD*)nullptr);
    const size_t img = (size_t)H * W * C;

    // group A: member (v, h), output row fh(y0 + i), pixels fv(x0 + nc - 1) .. fv(x0) or x0 .. x0 + nc - 1
    for (int e = tid; e < 4 * ENS_T * SLOTS; e += 256) {
        const int q = e % SLOTS, i = (e / SLOTS) % ENS_T, m = e / (SLOTS * ENS_T);
        if (i >= nr) continue;
        const int v = m & 1, h = m >> 1;
        const size_t r = h ? H - 1 - (y0 + i) : y0 + i, c0 = v ? W - x0 - nc : x0;
        TD* g = out_a + ((size_t)m * N + n) * img + (r * W + c0) * C;
        const TS* l = s_t + i * P + ((mis0 + i * misr) & 3);
        ens_store_slot(g, nc * C, q, [&](int k) {
            const int p = k / C, c = k - p * C;
            const int j = v ? nc - 1 - p : p;
            return ens_convert(l[j * C + (SWAP ? C - 1 - c : c)], (const TD*)nullptr);
        });
    }
    // group T: member (v, h), output row fv(x0 + j) of W rows, its pixels are the tile's rows (reversed by h)
    for (int e = tid; e < 4 * ENS_T * SLOTS; e += 256) {
        const int q = e % SLOTS, j = (e / SLOTS) % ENS_T, m = e / (SLOTS * ENS_T);
        if (j >= nc) continue;
        const int v = m & 1, h = m >> 1;
        const size_t r = v ? W - 1 - (x0 + j) : x0 + j, c0 = h ? H - y0 - nr : y0;
        TD* g = out_t + ((size_t)m * N + n) * img + (r * H + c0) * C;
        ens_store_slot(g, nr * C, q, [&](int k) {
            const int p = k / C, c = k - p * C;
            const int i = h ? nr - 1 - p : p;
            return ens_convert(s_t[i * P + ((mis0 + i * misr) & 3) + j * C + (SWAP ? C - 1 - c : c)], (const TD*)nullptr);
        });
    }
}

template <class TS, class TD>
static int ens_expand(const TS* src, TD* out_a, TD* out_t, int N, int H, int W, int C, int swap_rb, void* stream) {
    DASR_CHECK_PTR(src); DASR_CHECK_PTR(out_a); DASR_CHECK_PTR(out_t);
    DASR_CHECK_SHAPE(N > 0 && H > 0 && W > 0 && C > 0);
    if (C != 1 && C != 3) return DASR_E_UNSUPPORTED;
    DASR_CHECK_SHAPE(N <= 65535 && dasr_cdiv(H, ENS_T) <= 65535);
    const dim3 grid(dasr_cdiv(W, ENS_T), dasr_cdiv(H, ENS_T), N);
    if (C == 1)
        DASR_LAUNCH((k_ens_expand<TS, TD, 1, false>), grid, dim3(256), 0, stream, src, out_a, out_t, N, H, W);
    else if (swap_rb)
        DASR_LAUNCH((k_ens_expand<TS, TD, 3, true>), grid, dim3(256), 0, stream, src, out_a, out_t, N, H, W);
    else
        DASR_LAUNCH((k_ens_expand<TS, TD, 3, false>), grid, dim3(256), 0, stream, src, out_a, out_t, N, H, W);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_ensemble_expand_f32(const float* src, float* out_a, float* out_t, int N, int H, int W, int C,
                                        void* stream) {
    return ens_expand<float, float>(src, out_a, out_t, N, H, W, C, 0, stream);
}

extern "C" int dasr_ensemble_expand_u8(const unsigned char* src, unsigned char* out_a, unsigned char* out_t, int N, int H,
                                       int W, int C, void* stream) {
    return ens_expand<unsigned char, unsigned char>(src, out_a, out_t, N, H, W, C, 0, stream);
}

extern "C" int dasr_ensemble_ingest_u8(const unsigned char* frames, float* out_a, float* out_t, int N, int H, int W, int C,
                                       int swap_rb, void* stream) {
    return ens_expand<unsigned char, float>(frames, out_a, out_t, N, H, W, C, swap_rb, stream);
}

// ---- merge --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ens_clamp(float v, float lo, float hi) {
    return v != v ? v : fminf(fmaxf(v, lo), hi);        // torch.clamp keeps NaN (k_clamp_to_nchw)
}

// H x W: the OUTPUT image.  A thread owns the elements tid + 256 u of the tile (row i, pixel p, channel c; p and c fastest).
template <int C>
__global__ void __launch_bounds__(256) k_ens_merge(const float* __restrict__ y_a, const float* __restrict__ y_t,
                                                   float* __restrict__ out, int N, int H, int W, float lo, float hi) {
    constexpr int P = ens_lds<float, C>::pitch, ROW = ENS_T * C, PER = ENS_T * ROW / 256;
    __shared__ float s_t[ENS_T * P];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * ENS_T, x0 = blockIdx.x * ENS_T;
    const int nr = H - y0 < ENS_T ? H - y0 : ENS_T, nc = W - x0 < ENS_T ? W - x0 : ENS_T;
    const size_t img = (size_t)H * W * C;
    float acc[PER] = {};

    // members 0..3: z_m[r, c] = clamp(y_m[fh(r), fv(c)]), read in place (lanes run along a source row, backwards under v)
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int v = m & 1, h = m >> 1;
        const float* ym = y_a + ((size_t)m * N + n) * img;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u, i = e / ROW, k = e - i * ROW, p = k / C, c = k - p * C;
            if (i >= nr || p >= nc) continue;
            const size_t r = h ? H - 1 - (y0 + i) : y0 + i, cc = v ? W - 1 - (x0 + p) : x0 + p;
            const float z = ens_clamp(ym[(r * W + cc) * C + c], lo, hi);
            acc[u] = m == 0 ? z : ens_add(acc[u], z);
        }
    }
    // members 4..7: z_m[r, c] = clamp(y_m[fv(c), fh(r)]) of a [W,H] image: its rows fv(x0 .. x0+nc-1), pixels
    // fh(y0 .. y0+nr-1) of each, through LDS (loaded along those rows, read across them)
#pragma unroll 1
    for (int m = 0; m < 4; ++m) {
        const int v = m & 1, h = m >> 1;
        const size_t r0 = v ? W - x0 - nc : x0, c0 = h ? H - y0 - nr : y0;
        const float* ym = y_t + ((size_t)m * N + n) * img + (r0 * H + c0) * C;
        if (m) __syncthreads();
        for (int e = tid; e < ENS_T * ROW; e += 256) {
            const int j = e / ROW, k = e - j * ROW;
            if (j < nc && k < nr * C) s_t[j * P + k] = ym[(size_t)j * H * C + k];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + 256 * u, i = e / ROW, k = e - i * ROW, p = k / C, c = k - p * C;
            if (i >= nr || p >= nc) continue;
            const int j = v ? nc - 1 - p : p, ii = h ? nr - 1 - i : i;
            acc[u] = ens_add(acc[u], ens_clamp(s_t[j * P + ii * C + c], lo, hi));
        }
    }
    float* o = out + (size_t)n * img;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = tid + 256 * u, i = e / ROW, k = e - i * ROW, p = k / C, c = k - p * C;
        if (i >= nr || p >= nc) continue;
        o[((size_t)(y0 + i) * W + x0 + p) * C + c] = ens_mul(0.125f, acc[u]);
    }
}

extern "C" int dasr_ensemble_merge(const float* y_a, const float* y_t, float* out, int N, int H, int W, int C, float lo,
                                   float hi, void* stream) {
    DASR_CHECK_PTR(y_a); DASR_CHECK_PTR(y_t); DASR_CHECK_PTR(out);
    DASR_CHECK_SHAPE(N > 0 && H > 0 && W > 0 && C > 0);
    if (C != 1 && C != 3) return DASR_E_UNSUPPORTED;
    DASR_CHECK_SHAPE(N <= 65535 && dasr_cdiv(H, ENS_T) <= 65535);
    const dim3 grid(dasr_cdiv(W, ENS_T), dasr_cdiv(H, ENS_T), N);
    if (C == 1)
        DASR_LAUNCH(k_ens_merge<1>, grid, dim3(256), 0, stream, y_a, y_t, out, N, H, W, lo, hi);
    else
        DASR_LAUNCH(k_ens_merge<3>, grid, dim3(256), 0, stream, y_a, y_t, out, N, H, W, lo, hi);
    DASR_RETURN_LAUNCH_STATUS();
}
