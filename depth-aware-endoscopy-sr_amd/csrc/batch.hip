// batch.hip — training batches from uint8 HR frames: the image half of the reference's training loader on the device.
//
//   dasr_batch_lr_u8      uint8 [B,H,W,3] HWC BGR (the HR frames) -> float [B,3,h',w'] NCHW RGB, the LR image:
//                         read_img's `/ 255.` (data/util.py:71-84), imresize_np(img, 1/s, True) (data/util.py:258-458:
//                         cubic, calculate_weights_indices, imresize_np), an optional crop window of it, augment
//                         (data/util.py:101-118) and the BGR->RGB / HWC->CHW packing (LQGTker_Depth_dataset.py:145-199)
//   dasr_batch_gt_u8      the same frames -> float [B,3,Hc,Wc] NCHW RGB GT = u8 / 255 (IEEE division, the values of
//                         dasr_frame_ingest_u8) of the window s * (oy, ox), size s * (ch, cw), with the same augment
//   dasr_batch_plane_f32  float [B,C,h,w] -> the cropped and augmented [B,C,h',w'] (the depth map, the mask planes)
//   dasr_batch_plane_u8   the same gather with 1-byte elements (the region bytes of crop mode)
//
// Per-sample tables are DEVICE memory (int32 [B,2] crop origins (oy, ox) in LR pixels, uint8 [B] flags: bit 0 hflip,
// bit 1 vflip, bit 2 transpose), so a captured graph holds the chain and only the table contents change.  augment's order:
// img[:, ::-1], then img[::-1], then transpose(1, 0, 2): window pixel (y, x) of a (ch, cw) window lands at
// (y', x') = (vflip ? ch-1-y : y, hflip ? cw-1-x : x), and at (x', y') with the transpose (ch == cw then).
//
// Plain vector loads and stores, no atomics, no inline assembly.  An origin outside [0, h - ch] x [0, w - cw] is clamped
// into it and the index table entries are clamped to the staged tile: bad table CONTENTS give wrong pixels, never an access
// outside the buffers.
#include "dasr_common.h"

#if DASR_DEVICE_BUILD
__device__ __forceinline__ float batch_div(float a, float b) { return __fdiv_rn(a, b); }
#else
static inline float batch_div(float a, float b) { volatile float r = a / b; return r; }
#endif

#define BATCH_FLIP_H 1
#define BATCH_FLIP_V 2
#define BATCH_TRANSPOSE 4

// the window's origin of sample b, clamped into the frame
__device__ __forceinline__ void batch_origin(const int* __restrict__ origins, int b, int h, int w, int ch, int cw, int& oy,
                                             int& ox) {
    oy = origins ? origins[2 * b] : 0;
    ox = origins ? origins[2 * b + 1] : 0;
    oy = oy < 0 ? 0 : (oy > h - ch ? h - ch : oy);
    ox = ox < 0 ? 0 : (ox > w - cw ? w - cw : ox);
}

// where window pixel (y, x) of a (ch, cw) window goes: the offset inside one output plane
__device__ __forceinline__ size_t batch_dst(int y, int x, int ch, int cw, int flags) {
    const int yy = (flags & BATCH_FLIP_V) ? ch - 1 - y : y;
    const int xx = (flags & BATCH_FLIP_H) ? cw - 1 - x : x;
    return (flags & BATCH_TRANSPOSE) ? (size_t)xx * ch + yy : (size_t)yy * cw + xx;
}

// n bytes from g (any alignment) into the LDS row l (4-byte aligned) so that byte i lands at l[((uintptr_t)g & 3) + i]:
// aligned dwords of the source are aligned dwords of the row; the bytes before the first and after the last whole dword
// go one at a time.  Called by one wave (lane of 64).
__device__ __forceinline__ void batch_stage_row(const unsigned char* __restrict__ g, unsigned char* l, int n, int lane) {
    const int mis = (int)((uintptr_t)g & 3);
    int head = (4 - mis) & 3;
    if (head > n) head = n;
    const int body = (n - head) >> 2, tail = n - head - 4 * body;
    const unsigned* gs = (const unsigned*)(g + head);
    unsigned* ld = (unsigned*)(l + mis + head);
    for (int i = lane; i < body; i += 64) ld[i] = gs[i];
    for (int i = lane; i < head + tail; i += 64) {
        const int e = i < head ? i : head + 4 * body + (i - head);
        l[mis + e] = g[e];
    }
}

// symmetric, edge-including reflection (-1 -> 0, -2 -> 1, n -> n-1, ...), then relative to the staged range [c0, c0 + cn)
__device__ __forceinline__ int batch_reflect_rel(int idx, int n, int c0, int cn) {
    idx = idx < 0 ? -idx - 1 : idx;
    idx = idx >= n ? 2 * n - 1 - idx : idx;
    idx -= c0;
    return idx < 0 ? 0 : (idx >= cn ? cn - 1 : idx);
}

// ---- LR: antialiased bicubic of the uint8 frame ----------------------------------------------------------------------
// One workgroup = one TH x TW tile of a sample's LR window.  The HR rows and columns its taps touch (clipped to the frame:
// the reflected ones lie inside the clipped range) are staged as uint8, the H pass leaves fp32 [TH][columns * 3] in LDS
// (the reference rounds its H pass to fp32 too), the W pass writes the outputs.  Every output is one fmaf chain over its
// 4s taps in tap order, in both passes: its bits do not depend on the tile, the grid, the window or the batch.  The index
// tables must be non-decreasing (the staged range runs from the first output's first tap to the last output's last).
#define LR_MAX_S 8
#define LR_MAX_ROWS 88                  // (TH - 1) s + 4 s            at most, over the four tile shapes below
#define LR_MAX_COLS 152                 // (TW - 1) s + 4 s
#define LR_STRIDE 460                   // 3 LR_MAX_COLS + 3 bytes of misalignment, rounded up to a dword
#define LR_MAX_MID 3664                 // TH * (3 * columns | 1): the row pitch of the intermediate is odd
#define LR_MAX_WH 256                   // TH * 4 s
#define LR_MAX_WW 512                   // TW * 4 s

struct BatchLrArgs {
    const unsigned char* frames;
    float* out;
    const float *wh, *ww;
    const int *ih, *iw;
    const int* origins;
    const unsigned char* flags;
    int H, W, s, h, w, ch, cw, TH, TW, mask;
};

__global__ void __launch_bounds__(256) k_batch_lr_u8(BatchLrArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_u8[LR_MAX_ROWS * LR_STRIDE];
    __shared__ float s_mid[LR_MAX_MID];
    __shared__ float s_wh[LR_MAX_WH], s_ww[LR_MAX_WW];
    __shared__ int s_ih[16], s_iw[32];

    const int b = blockIdx.z, tid = threadIdx.x;
    const int s = a.s, taps = 4 * s;
    int oy, ox;
    batch_origin(a.origins, b, a.h, a.w, a.ch, a.cw, oy, ox);
    const int flags = (a.flags ? a.flags[b] : 0) & a.mask;
    const int y0 = blockIdx.y * a.TH, x0 = blockIdx.x * a.TW;                     // tile origin inside the window
    const int nr = a.ch - y0 < a.TH ? a.ch - y0 : a.TH, nc = a.cw - x0 < a.TW ? a.cw - x0 : a.TW;
    const int r0 = oy + y0, c0 = ox + x0;                                         // ... inside the full LR image

    // the HR rows / columns of the tile's taps, clipped to the frame and to the staging buffers
    int ya = a.ih[r0], yb = a.ih[r0 + nr - 1] + taps;
    int xa = a.iw[c0], xb = a.iw[c0 + nc - 1] + taps;
    ya = ya < 0 ? 0 : (ya > a.H - 1 ? a.H - 1 : ya);
    xa = xa < 0 ? 0 : (xa > a.W - 1 ? a.W - 1 : xa);
    yb = yb > a.H ? a.H : yb;
    xb = xb > a.W ? a.W : xb;
    int ny = yb - ya, nx = xb - xa;
    const int ymax = (a.TH - 1) * s + taps, xmax = (a.TW - 1) * s + taps;         // what sane tables ask for at most
    ny = ny < 1 ? 1 : (ny > ymax ? ymax : ny);
    nx = nx < 1 ? 1 : (nx > xmax ? xmax : nx);
    const int nb = 3 * nx;                                                        // staged bytes per row
    const int np = nb | 1;                                                        // row pitch of the fp32 intermediate

    const size_t rowbytes = (size_t)a.W * 3;
    const unsigned char* src = a.frames + (size_t)b * a.H * rowbytes + (size_t)xa * 3;
    for (int r = tid >> 6; r < ny; r += 4)
        batch_stage_row(src + (size_t)(ya + r) * rowbytes, s_u8 + r * LR_STRIDE, nb, tid & 63);
    for (int i = tid; i < nr * taps; i += 256) s_wh[i] = a.wh[(size_t)(r0 + i / taps) * taps + i % taps];
    for (int i = tid; i < nc * taps; i += 256) s_ww[i] = a.ww[(size_t)(c0 + i / taps) * taps + i % taps];
    if (tid < nr) s_ih[tid] = a.ih[r0 + tid];
    if (tid >= 64 && tid - 64 < nc) s_iw[tid - 64] = a.iw[c0 + tid - 64];
    __syncthreads();

    // H pass: s_mid[i][cb] = sum_k wh[r0+i][k] * (u8[reflect(ih[r0+i] + k)][cb] / 255), k ascending.
    const int mis0 = (int)((uintptr_t)src & 3), misr = (int)(rowbytes & 3);
    bool regular = true;                                       // consecutive outputs start s rows apart (resize_tables' do)
    for (int i = 1; i < nr; ++i) regular = regular && s_ih[i] == s_ih[0] + i * s;
    if (regular) {
        // A thread owns a column byte and walks the tile's HR rows once, in blocks of s: the row of block q, position t is
        // tap (q - i) s + t of the outputs i = q-3 .. q.  Four accumulators in flight, the oldest is complete after each
        // block.  One byte -> float conversion and division per HR sample instead of four; every output still sums its
        // taps in ascending order from zero, so the bits are those of the loop below.
        const int first0 = s_ih[0];
        for (int cb = tid; cb < nb; cb += 256) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;      // outputs q, q-1, q-2, q-3
            for (int q = 0; q < nr + 3; ++q) {
                const float* w0 = s_wh + (q < nr ? q : 0) * taps;
                const float* w1 = s_wh + (q >= 1 && q - 1 < nr ? q - 1 : 0) * taps + s;
                const float* w2 = s_wh + (q >= 2 && q - 2 < nr ? q - 2 : 0) * taps + 2 * s;
                const float* w3 = s_wh + (q >= 3 ? q - 3 : 0) * taps + 3 * s;
                for (int k = 0; k < s; ++k) {
                    const int rel = batch_reflect_rel(first0 + q * s + k, a.H, ya, ny);
                    const int mis = (mis0 + (ya + rel) * misr) & 3;
                    const float v = batch_div((float)s_u8[rel * LR_STRIDE + mis + cb], 255.0f);
                    a0 = fmaf(w0[k], v, a0);
                    a1 = fmaf(w1[k], v, a1);
                    a2 = fmaf(w2[k], v, a2);
                    a3 = fmaf(w3[k], v, a3);
                }
                if (q >= 3) s_mid[(q - 3) * np + cb] = a3;     // (an accumulator of an output outside 0 .. nr-1 is never stored)
                a3 = a2; a2 = a1; a1 = a0; a0 = 0.f;
            }
        }
    } else {
        for (int e = tid; e < nr * nb; e += 256) {
            const int i = e / nb, cb = e - i * nb;
            const int first = s_ih[i];
            const float* wrow = s_wh + i * taps;
            float acc = 0.f;
            for (int k = 0; k < taps; ++k) {
                const int rel = batch_reflect_rel(first + k, a.H, ya, ny);
                const int mis = (mis0 + (ya + rel) * misr) & 3;
                const float v = batch_div((float)s_u8[rel * LR_STRIDE + mis + cb], 255.0f);
                acc = fmaf(wrow[k], v, acc);
            }
            s_mid[i * np + cb] = acc;
        }
    }
    __syncthreads();

    // W pass, augment, BGR -> RGB
    const size_t plane = (size_t)a.ch * a.cw;
    float* out = a.out + (size_t)b * 3 * plane;
    // rows fastest across the lanes: a tap reads s_mid[i * np + 3 * column + c], and with lanes along a row the 3 s floats
    // between neighbouring outputs put a wave on 4 (x8) or 8 banks; np is odd, so lanes that differ in i differ in bank
    for (int e = tid; e < nr * nc * 3; e += 256) {
        const int i = e % nr, p = e / nr;
        const int j = p % nc, c = p / nc;
        const int first = s_iw[j];
        const float* wrow = s_ww + j * taps;
        const float* mrow = s_mid + i * np + c;
        float acc = 0.f;
        for (int k = 0; k < taps; ++k) acc = fmaf(wrow[k], mrow[3 * batch_reflect_rel(first + k, a.W, xa, nx)], acc);
        out[(size_t)(2 - c) * plane + batch_dst(y0 + i, x0 + j, a.ch, a.cw, flags)] = acc;
    }
}

// a side must hold the reflection of the first and last outputs' taps: floor(0.5 + 1.5 s) samples (12 / 6 / 5 / 3 for
// s = 8 / 4 / 3 / 2); the reference's index_select raises on shorter ones
static int batch_reflect_len(int s) { return (3 * s + 1) / 2; }

extern "C" int dasr_batch_lr_u8(const unsigned char* frames, float* lr, const float* wh, const int* ih, const float* ww,
                                const int* iw, const int* origins, const unsigned char* flags, int B, int H, int W, int s,
                                int ch, int cw, int allow_transpose, void* stream) {
    DASR_CHECK_PTR(frames); DASR_CHECK_PTR(lr); DASR_CHECK_PTR(wh); DASR_CHECK_PTR(ih); DASR_CHECK_PTR(ww); DASR_CHECK_PTR(iw);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && ch > 0 && cw > 0 && B <= 65535);
    if (s != 2 && s != 3 && s != 4 && s != 8) return DASR_E_UNSUPPORTED;
    DASR_CHECK_SHAPE(H % s == 0 && W % s == 0 && H >= batch_reflect_len(s) && W >= batch_reflect_len(s));
    DASR_CHECK_SHAPE(ch <= H / s && cw <= W / s && dasr_cdiv(ch, 8) <= 65535);
    DASR_CHECK_SHAPE(!allow_transpose || ch == cw);
    // with allow_transpose == 0 the transpose bit of a flag is ignored (the caller says its flags do not carry it)
    BatchLrArgs a = {frames, lr, wh, ww, ih, iw, origins, flags, H, W, s, H / s, W / s, ch, cw, s == 8 ? 8 : 16, s == 2 ? 32 : 16,
                     allow_transpose ? 7 : 3};
    DASR_LAUNCH(k_batch_lr_u8, dim3(dasr_cdiv(cw, a.TW), dasr_cdiv(ch, a.TH), B), dim3(256), 0, stream, a);
    DASR_RETURN_LAUNCH_STATUS();
}

// ---- GT: u8 / 255 of the HR window, augmented, NCHW RGB -----------------------------------------------------------------
// One workgroup = 32 rows x 64 pixels of the window: 192 bytes per row into LDS (row pitch 200 bytes = 50 dwords: the 32
// rows a wave reads for a transposed store fall on 32 different banks), then one store instruction per 64 consecutive
// floats of an output row (untransposed: 64 pixels of a source row, reversed by hflip; transposed: 2 x 32 pixels of two source
// columns, each a full 128-byte line).
#define GT_TY 32
#define GT_TX 64
#define GT_PITCH 200

__global__ void __launch_bounds__(256) k_batch_gt_u8(const unsigned char* __restrict__ frames, float* __restrict__ gt,
                                                     const int* __restrict__ origins, const unsigned char* __restrict__ flags,
                                                     int H, int W, int s, int ch, int cw, int mask) {
    __shared__ __attribute__((aligned(16))) unsigned char s_u8[GT_TY * GT_PITCH];
    const int b = blockIdx.z, tid = threadIdx.x;
    int oy, ox;
    batch_origin(origins, b, H / s, W / s, ch, cw, oy, ox);
    const int fl = (flags ? flags[b] : 0) & mask;
    const int Hc = s * ch, Wc = s * cw;
    const int y0 = blockIdx.y * GT_TY, x0 = blockIdx.x * GT_TX;
    const int nr = Hc - y0 < GT_TY ? Hc - y0 : GT_TY, nc = Wc - x0 < GT_TX ? Wc - x0 : GT_TX;
    const size_t rowbytes = (size_t)W * 3;
    const unsigned char* src = frames + ((size_t)b * H + (size_t)s * oy + y0) * rowbytes + ((size_t)s * ox + x0) * 3;
    for (int r = tid >> 6; r < nr; r += 4) batch_stage_row(src + (size_t)r * rowbytes, s_u8 + r * GT_PITCH, 3 * nc, tid & 63);
    __syncthreads();
    const int mis0 = (int)((uintptr_t)src & 3), misr = (int)(rowbytes & 3);
    const size_t plane = (size_t)Hc * Wc;
    float* out = gt + (size_t)b * 3 * plane;
    if (!(fl & BATCH_TRANSPOSE)) {
        // lane = output column inside the tile; ascending output addresses whatever hflip says
        for (int e = tid; e < 3 * GT_TY * GT_TX; e += 256) {
            const int l = e & (GT_TX - 1), i = (e >> 6) & (GT_TY - 1), c = e >> 11;
            if (i >= nr || l >= nc) continue;
            const int j = (fl & BATCH_FLIP_H) ? nc - 1 - l : l;
            const int mis = (mis0 + i * misr) & 3;
            out[(size_t)(2 - c) * plane + batch_dst(y0 + i, x0 + j, Hc, Wc, fl)] =
                batch_div((float)s_u8[i * GT_PITCH + mis + 3 * j + c], 255.0f);
        }
    } else {
        // output rows are source columns: lane = source row inside the tile (reversed by vflip)
        for (int e = tid; e < 3 * GT_TY * GT_TX; e += 256) {
            const int l = e & (GT_TY - 1), j = (e >> 5) & (GT_TX - 1), c = e >> 11;
            if (l >= nr || j >= nc) continue;
            const int i = (fl & BATCH_FLIP_V) ? nr - 1 - l : l;
            const int mis = (mis0 + i * misr) & 3;
            out[(size_t)(2 - c) * plane + batch_dst(y0 + i, x0 + j, Hc, Wc, fl)] =
                batch_div((float)s_u8[i * GT_PITCH + mis + 3 * j + c], 255.0f);
        }
    }
}

extern "C" int dasr_batch_gt_u8(const unsigned char* frames, float* gt, const int* origins, const unsigned char* flags, int B,
                                int H, int W, int s, int ch, int cw, int allow_transpose, void* stream) {
    DASR_CHECK_PTR(frames); DASR_CHECK_PTR(gt);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && s > 0 && ch > 0 && cw > 0 && B <= 65535);
    DASR_CHECK_SHAPE(H % s == 0 && W % s == 0 && ch <= H / s && cw <= W / s);
    DASR_CHECK_SHAPE(!allow_transpose || ch == cw);
    DASR_CHECK_SHAPE(dasr_cdiv((size_t)s * ch, GT_TY) <= 65535);
    DASR_LAUNCH(k_batch_gt_u8, dim3(dasr_cdiv((size_t)s * cw, GT_TX), dasr_cdiv((size_t)s * ch, GT_TY), B), dim3(256), 0, stream,
                frames, gt, origins, flags, H, W, s, ch, cw, allow_transpose ? 7 : 3);
    DASR_RETURN_LAUNCH_STATUS();
}

// ---- planes: crop + augment of [B,C,h,w] ------------------------------------------------------------------------------------
// One workgroup = a 32 x 32 tile of one plane's window through LDS (pitch 33): loads run along source rows, stores along
// output rows, for all eight flag values.
template <class T>
__global__ void __launch_bounds__(256) k_batch_plane(const T* __restrict__ in, T* __restrict__ out,
                                                     const int* __restrict__ origins, const unsigned char* __restrict__ flags,
                                                     int C, int h, int w, int ch, int cw, int mask) {
    __shared__ T s_t[32 * 33];
    const int bc = blockIdx.z, b = bc / C, tid = threadIdx.x;
    int oy, ox;
    batch_origin(origins, b, h, w, ch, cw, oy, ox);
    const int fl = (flags ? flags[b] : 0) & mask;
    const int y0 = blockIdx.y * 32, x0 = blockIdx.x * 32;
    const int nr = ch - y0 < 32 ? ch - y0 : 32, nc = cw - x0 < 32 ? cw - x0 : 32;
    const T* src = in + ((size_t)bc * h + oy + y0) * w + ox + x0;
    for (int e = tid; e < 32 * 32; e += 256) {
        const int i = e >> 5, j = e & 31;
        if (i < nr && j < nc) s_t[i * 33 + j] = src[(size_t)i * w + j];
    }
    __syncthreads();
    T* dst = out + (size_t)bc * ch * cw;
    for (int e = tid; e < 32 * 32; e += 256) {
        const int l = e & 31, m = e >> 5;             // l: along the output row
        int i, j;
        if (fl & BATCH_TRANSPOSE) {
            j = m;
            i = (fl & BATCH_FLIP_V) ? nr - 1 - l : l;
        } else {
            i = m;
            j = (fl & BATCH_FLIP_H) ? nc - 1 - l : l;
        }
        if (i < 0 || j < 0 || i >= nr || j >= nc) continue;
        dst[batch_dst(y0 + i, x0 + j, ch, cw, fl)] = s_t[i * 33 + j];
    }
}

template <class T>
static int batch_plane(const T* in, T* out, const int* origins, const unsigned char* flags, int B, int C, int h, int w, int ch,
                       int cw, int allow_transpose, void* stream) {
    DASR_CHECK_PTR(in); DASR_CHECK_PTR(out);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && ch > 0 && cw > 0 && ch <= h && cw <= w);
    DASR_CHECK_SHAPE(!allow_transpose || ch == cw);
    DASR_CHECK_SHAPE((size_t)B * C <= 65535 && dasr_cdiv(ch, 32) <= 65535);
    DASR_LAUNCH(k_batch_plane<T>, dim3(dasr_cdiv(cw, 32), dasr_cdiv(ch, 32), B * C), dim3(256), 0, stream, in, out, origins,
                flags, C, h, w, ch, cw, allow_transpose ? 7 : 3);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_batch_plane_f32(const float* in, float* out, const int* origins, const unsigned char* flags, int B, int C,
                                    int h, int w, int ch, int cw, int allow_transpose, void* stream) {
    return batch_plane<float>(in, out, origins, flags, B, C, h, w, ch, cw, allow_transpose, stream);
}

extern "C" int dasr_batch_plane_u8(const unsigned char* in, unsigned char* out, const int* origins, const unsigned char* flags,
                                   int B, int C, int h, int w, int ch, int cw, int allow_transpose, void* stream) {
    return batch_plane<unsigned char>(in, out, origins, flags, B, C, h, w, ch, cw, allow_transpose, stream);
}
