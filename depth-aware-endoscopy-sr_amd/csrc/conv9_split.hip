// conv9_split.hip — the generator's 9x9 output convolution (conv_output, sftmd_arch.py:910,948: 32 -> 3 channels at HR
// resolution) of the FP32 path on the fp16 matrix cores, at fp32 accuracy: the "split fp16 x 2" scheme of conv_split_bf16.hip
// (two fp16 pieces per operand scaled by a power of two taken from the tensor's max |.|, three MFMA products per term, fp32
// accumulation) on the folding of conv9_mfma.hip / conv9_bf16_mfma.hip (one kernel axis goes into N: an MFMA tile is 27/32
// full).  The exact-fp32 MFMA kernels it replaces ran at 79 / 108 / 95 TF (forward / dgrad / wgrad: 11 ms of the 77 ms x8
// step); here the matrix work is 3/16 of theirs.
//   forward:  P[q][(kw,co)] = sum_{kh,ci} x[q.y+kh-4, q.x][ci] * w[kh][kw][ci][co]        M = pixels q, N = 27, K = 9*Cin
//             y[p][co]      = bias[co] + sum_kw P[(p.y, p.x+kw-4)][(kw,co)]                 (9-term shift-add via LDS, fp32)
//   dgrad:    dx[q][ci]     = sum_kh sum_k' E[q.y-kh+4][q.x][k'] * Wd[kh][k'][ci]            M = pixels, N = 32 ci, K = 9*32
//   wgrad:    dW[kh][k'][ci] = sum_q x[q][ci] * E[q.y-kh+4][q.x][k']                         M = ci, N = 27, K = pixels
// with k' = Cout*(8-kw) + co and E[row][px][k'] = the 27 consecutive values of the 3-channel dy row starting at pixel px-4.
// Everything that is an MFMA operand lives in LDS as TWO fp16 images (value and what the first rounding left), so tiles are
// half the size of the bf16 kernels': the forward walks 16-channel chunks of an 8 x 24 pixel tile (its first form: 8 x 56), the
// wgrad 8 x 32 tiles, the dgrad 8 x 16 tiles.  All three kernels are persistent (forward and dgrad: two 256-thread workgroups
// per CU whose phases overlap, wgrad: one of 512; kernel images staged once) and hold the next tile's global loads in
// registers while the current one is multiplied.
#include "bf16.h"
#include "conv_kernels.h"

typedef _Float16 h16_t;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

#define S9_TH 8                       // tile rows

struct Conv9SplitArgs {
    const float* x;      // fwd / wgrad: [B,H,W,Cin]
    const float* w;      // HWIO [9][9][Cin][Cout]
    const float* bias;   // fwd
    const float* dy;     // dgrad / wgrad: [B,H,W,Cout]
    void* out;           // fwd: y; dgrad: dx; wgrad: slabs
    const float* xmax;   // amax buffers (dasr_common.h): x (fwd / wgrad), dy (dgrad / wgrad) ...
    const float* dmax;
    const float* wmax;   // ... and the kernel (fwd / dgrad)
    int B, H, W, Cin, Cout;
    int accumulate, P, ntiles;
    const float* xact;   // fused dgrad: the convolution's saved input (the producer's activated, shuffled output) ...
    float* amax;         // ... the amax buffer of dprev (may be NULL) ...
    int act;             // ... and the producer's activation
};

// ---- scales: the maximum of an amax buffer's parts, by the whole workgroup (phase 1 before a barrier, phase 2 after it)
__device__ __forceinline__ float s9_amax_share(const float* buf) {
    float m = 0.f;
    if (buf) {
        int n;
        memcpy(&n, buf, 4);
        for (int i = threadIdx.x; i < n; i += blockDim.x) m = fmaxf(m, buf[1 + i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}
__host__ __device__ static inline int s9_scale_exp(float m) {      // 2^k puts m in [2^14, 2^15); k clamped to [-60, 60]
    unsigned u;
    memcpy(&u, &m, 4);
    int k = 14 - ((int)((u >> 23) & 0xffu) - 127);
    return k < -60 ? -60 : (k > 60 ? 60 : k);
}
__host__ __device__ static inline float s9_pow2(int k) {
    const unsigned u = (unsigned)(127 + k) << 23;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// a, b: the two amax buffers of the launch; returns their scale exponents through s_red ([32] floats of LDS)
__device__ __forceinline__ void s9_scales(const float* a, const float* b, float* s_red, int& ka, int& kb) {
    const float ma = s9_amax_share(a), mb = s9_amax_share(b);
    if ((threadIdx.x & 63) == 0) {
        s_red[threadIdx.x >> 6] = ma;
        s_red[16 + (threadIdx.x >> 6)] = mb;
    }
    __syncthreads();
    float xa = s_red[0], xb = s_red[16];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { xa = fmaxf(xa, s_red[w]); xb = fmaxf(xb, s_red[16 + w]); }
    ka = s9_scale_exp(xa);
    kb = s9_scale_exp(xb);
}
// v s = h0 + h1 to 22-23 bits
__device__ __forceinline__ void s9_split(float v, float s, h16_t& h0, h16_t& h1) {
    v *= s;
    h0 = (h16_t)v;
    h1 = (h16_t)(v - (float)h0);
}
__device__ __forceinline__ f32x16 s9_mma(const h16x8& a0, const h16x8& a1, const h16x8& b0, const h16x8& b1, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, c, 0, 0, 0);       // smallest terms first
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, c, 0, 0, 0);
    return c;
}

// ------------------------------------------------------------------------------------------ forward, first form
// (dasr_set_conv_bf16_impl(+ 8192), and every Cin other than 32: A/B runs and the equality test of the form below)
// 512 threads, tile = 8 rows x 56 columns of y (input tile 16 x 64 pixels), wave w owns tile row w (two 32-pixel M-tiles).
// K loop: 16-channel chunks; per chunk 9 kh x 2 M-tiles x 3 products = 54 MFMAs per wave.  LDS: two input images
// [16*64 px][24] fp16 (48-byte pixel stride: conflict-free ds_read_b128), the kernel [Cin/16][9 kh][32 n][24] x 2, the P
// image [8][64][28] fp32 aliasing the input.
#define S9F_TQ 64
#define S9F_ST 24
#define S9F_PST 28
__global__ void __launch_bounds__(512) k_conv9_fwd_split_1wg(Conv9SplitArgs a) {
    DASR_DYN_SMEM(smem);
    constexpr int NPX = (S9_TH + 8) * S9F_TQ;                      // 1024 staged pixels
    h16_t* sIn0 = (h16_t*)smem;                                    // [NPX][S9F_ST]
    h16_t* sIn1 = sIn0 + NPX * S9F_ST;
    const int NCK = a.Cin / 16;
    h16_t* sW0 = sIn1 + NPX * S9F_ST;                              // [NCK][9][32][S9F_ST]
    h16_t* sW1 = sW0 + NCK * 9 * 32 * S9F_ST;
    float* s_red = (float*)(sW1 + NCK * 9 * 32 * S9F_ST);          // [32]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int TWO = S9F_TQ - 8;
    const int tiles_x = (a.W + TWO - 1) / TWO, tiles_y = (a.H + S9_TH - 1) / S9_TH;
    const int total = tiles_x * tiles_y * a.B;
    const int NN = 9 * a.Cout;   // <= 27
    int kx, kw_;
    s9_scales(a.xmax, a.wmax, s_red, kx, kw_);
    const float sx = s9_pow2(kx), sw = s9_pow2(kw_), inv = s9_pow2(-(kx + kw_));
    // kernel images, once: sW[c][kh][n = kw*Cout+co][ci] (zero rows for n >= 9*Cout)
    for (int c = 0; c < NCK; ++c) {
        float wq[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int e = tid + 512 * u, ci = e & 15, n = (e >> 4) & 31, kh = e >> 9;
            const int nn = n < NN ? n : 0, kw = nn / a.Cout, co = nn % a.Cout;
            const float v = a.w[(((size_t)kh * 9 + kw) * a.Cin + 16 * c + ci) * a.Cout + co];
            wq[u] = n < NN ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            const int e = tid + 512 * u, ci = e & 15, n = (e >> 4) & 31, kh = e >> 9;
            h16_t h0, h1;
            s9_split(wq[u], sw, h0, h1);
            sW0[((c * 9 + kh) * 32 + n) * S9F_ST + ci] = h0;
            sW1[((c * 9 + kh) * 32 + n) * S9F_ST + ci] = h1;
        }
    }
    constexpr int NPC = NPX * 4 / 512;                             // 8 pieces of 16 bytes (4 channels) per thread and chunk
    u32x4_t vin[NPC];
    // loads of (tile, 16-channel chunk c0): unconditional (a tile index past the end re-reads the last tile)
    auto fetch = [&](int tile, int c0) {
        const int b = tile / (tiles_x * tiles_y), tt = tile - b * (tiles_x * tiles_y);
        const int x0 = (tt % tiles_x) * TWO, y0 = (tt / tiles_x) * S9_TH;
        const BufRsrc rx = dasr_make_rsrc(a.x + (size_t)b * a.H * a.W * a.Cin, (size_t)a.H * a.W * a.Cin * sizeof(float));
#pragma unroll
        for (int u = 0; u < NPC; ++u) {
            const int idx = tid + 512 * u, pix = idx >> 2, q4 = idx & 3;
            const int gy = y0 - 4 + pix / S9F_TQ, gx = x0 - 4 + pix % S9F_TQ;
            const unsigned off = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                                     ? (unsigned)(((gy * a.W + gx) * a.Cin + c0 + 4 * q4) * (int)sizeof(float)) : DASR_OOB;
            vin[u] = dasr_buffer_load16(rx, off);
        }
    };
    // Which tile a (workgroup, trip) slot works on.  a.P == 0: slot s = tile s.  a.P == 1 (256 workgroups, dealt to the eight
    // XCDs round robin): the 32 workgroups of an XCD take a 4 x 8 block of tiles per trip, so that the halo rows and columns a
    // tile shares with its neighbours (16 x 64 input pixels per 8 x 56 outputs: 2.3 x the bytes) are re-read from that XCD's L2
    // while they are hot instead of from another XCD's tile in flight at the same time.
    const int nbx = (tiles_x + 7) / 8, nby = (tiles_y + 3) / 4;
    const int nslots = a.P == 1 ? ((a.B * nbx * nby + 7) / 8) * 256 : total;
    auto slot_tile = [&](int s) {
        if (a.P != 1) return s;
        const int xcd = s & 7, j = (s >> 3) & 31, g = (s >> 8) * 8 + xcd;
        const int bimg = g / (nbx * nby), r = g - bimg * (nbx * nby);
        const int ty = (r / nbx) * 4 + (j >> 3), tx = (r % nbx) * 8 + (j & 7);
        return (bimg < a.B && ty < tiles_y && tx < tiles_x) ? (bimg * tiles_y + ty) * tiles_x + tx : -1;
    };
    auto next_slot = [&](int s) {                     // the next slot of this workgroup that holds a tile (or nslots)
        for (s += gridDim.x; s < nslots && slot_tile(s) < 0; s += gridDim.x) {}
        return s;
    };
    int slot = (int)blockIdx.x < nslots && slot_tile(blockIdx.x) >= 0 ? (int)blockIdx.x : next_slot(blockIdx.x);
    if (slot < nslots) fetch(slot_tile(slot), 0);
    for (; slot < nslots;) {
        const int tile = slot_tile(slot);
        const int nslot = next_slot(slot);
        const int b = tile / (tiles_x * tiles_y), tt = tile - b * (tiles_x * tiles_y);
        const int x0 = (tt % tiles_x) * TWO, y0 = (tt / tiles_x) * S9_TH;
        f32x16 acc[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        for (int c = 0; c < NCK; ++c) {
            __syncthreads();                               // every wave is done with the previous chunk / tile (incl. its P image)
#pragma unroll
            for (int u = 0; u < NPC; ++u) {
                const int idx = tid + 512 * u;
                float f[4];
                memcpy(f, &vin[u], 16);
                h16x4 p0, p1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    h16_t h0, h1;
                    s9_split(f[j], sx, h0, h1);
                    p0[j] = h0; p1[j] = h1;
                }
                *(h16x4*)(sIn0 + (idx >> 2) * S9F_ST + 4 * (idx & 3)) = p0;
                *(h16x4*)(sIn1 + (idx >> 2) * S9F_ST + 4 * (idx & 3)) = p1;
            }
            __syncthreads();
            {                                              // next chunk of this tile, or the first chunk of the next tile
                const bool lastc = c + 1 == NCK;
                const int nt = nslot < nslots ? slot_tile(nslot) : tile;
                fetch(lastc ? nt : tile, lastc ? 0 : 16 * (c + 1));
            }
            const int wo = c * 9 * 32 * S9F_ST;
#pragma unroll
            for (int kh = 0; kh < 9; ++kh) {
                const h16x8 B0 = *(const h16x8*)(sW0 + wo + (kh * 32 + li) * S9F_ST + 8 * lh);
                const h16x8 B1 = *(const h16x8*)(sW1 + wo + (kh * 32 + li) * S9F_ST + 8 * lh);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int o = ((wv + kh) * S9F_TQ + 32 * m + li) * S9F_ST + 8 * lh;
                    const h16x8 A0 = *(const h16x8*)(sIn0 + o), A1 = *(const h16x8*)(sIn1 + o);
                    acc[m] = s9_mma(A0, A1, B0, B1, acc[m]);
                }
            }
        }
        __syncthreads();
        float* sP = (float*)smem;   // [8][64][PST]
        if (li < S9F_PST) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int qx = 32 * m + (g & 3) + 8 * (g >> 2) + 4 * lh;
                    sP[(wv * S9F_TQ + qx) * S9F_PST + li] = acc[m][g];
                }
        }
        __syncthreads();
        const int nout = S9_TH * TWO * a.Cout;
        float* y = (float*)a.out;
        for (int idx = tid; idx < nout; idx += 512) {
            const int co = idx % a.Cout, ox = (idx / a.Cout) % TWO, r = idx / (a.Cout * TWO);
            const int gy = y0 + r, gx = x0 + ox;
            if (gy >= a.H || gx >= a.W) continue;
            float v = 0.f;
#pragma unroll
            for (int kw = 0; kw < 9; ++kw) v += sP[(r * S9F_TQ + ox + kw) * S9F_PST + kw * a.Cout + co];
            y[(((size_t)b * a.H + gy) * a.W + gx) * a.Cout + co] = fmaf(v, inv, a.bias ? a.bias[co] : 0.f);
        }
        slot = nslot;
    }
}

// ------------------------------------------------------------------------------------------ forward (Cin = 32)
// 256 threads, TWO workgroups per CU (68.1 KB of LDS each) whose phases overlap: while one stages a chunk, writes its P image
// or does the shift-add, the other multiplies.  tile = 8 rows x 24 columns of y (input tile 16 x 32 pixels); wave w owns tile
// rows 2w, 2w+1 as two 32-pixel M-tiles.  Per 16-channel chunk and kh the two M-tiles take input rows 2w+kh and 2w+kh+1, so a
// row's fragment serves (kh, upper tile row) and (kh-1, lower): 10 A and 9 B fragment pairs per chunk for 54 MFMAs, read one
// kh ahead.  The order of the products of every output element is the first form's (chunk, kh, s9_mma's three, then the
// shift-add over kw from 0, then fmaf(v, inv, bias)): the two forms give the same bits.
// LDS: the input chunk as 2 x [16*32 px][16 ch] fp16 (32-byte pixel stride, the 16-byte piece index XORed with (px >> 3) & 1),
// the kernel as 2 x [9 kh][32 n][32 ci] (64-byte stride, piece index XORed with (n >> 2) & 3, as the dgrad's Wd): each 16-lane
// group of a ds_read_b128 meets every 16-byte slot of a bank row once.  The P image [8][32][28] fp32 aliases the input chunk.
// What does not depend on the tile - the staged pieces' pixel and LDS address, the shift-add's output -> (row, column, co)
// map with its divisions by Cout - is computed once per thread.  Loads and stores go through range-checked descriptors (out
// of the image and ragged tiles: DASR_OOB), every barrier is LDS-only: a tile's stores drain under the next tile's work and
// the next chunk's loads stay in flight across the MFMA phase.
#define S9G_TQ 32                      // staged columns
#define S9G_TWO (S9G_TQ - 8)           // output columns of a tile
#define S9G_PST 28
constexpr int S9G_NPX = (S9_TH + 8) * S9G_TQ;                      // 512 staged pixels
constexpr size_t S9G_LDS = sizeof(h16_t) * (size_t)(2 * S9G_NPX * 16 + 2 * 9 * 32 * 32) + 128;
static_assert(2 * S9G_LDS <= 160 * 1024, "two workgroups per CU");
static_assert(sizeof(float) * S9_TH * S9G_TQ * S9G_PST <= sizeof(h16_t) * 2 * S9G_NPX * 16, "the P image fits the input chunk");
constexpr int S9G_NOUT = (S9_TH * S9G_TWO * 3 + 255) / 256;        // shift-add trips of 256 threads (Cout <= 3)
__global__ void __launch_bounds__(256, 2) k_conv9_fwd_split(Conv9SplitArgs a) {
    DASR_DYN_SMEM(smem);
    h16_t* sIn0 = (h16_t*)smem;                                    // [512 px][16], pieces swizzled
    h16_t* sIn1 = sIn0 + S9G_NPX * 16;
    h16_t* sW0 = sIn1 + S9G_NPX * 16;                              // [9 kh][32 n][32 ci], pieces swizzled
    h16_t* sW1 = sW0 + 9 * 32 * 32;
    float* s_red = (float*)(sW1 + 9 * 32 * 32);                    // [32]
    const int tid = threadIdx.x, lane = tid & 63, wv = DASR_UNIFORM((int)(tid >> 6)), li = lane & 31, lh = lane >> 5;
    const int tiles_x = (a.W + S9G_TWO - 1) / S9G_TWO, tiles_y = (a.H + S9_TH - 1) / S9_TH;
    const int total = tiles_x * tiles_y * a.B;
    const int NN = 9 * a.Cout;   // <= 27
    int kx, kw_;
    s9_scales(a.xmax, a.wmax, s_red, kx, kw_);
    const float sx = s9_pow2(kx), sw = s9_pow2(kw_), inv = s9_pow2(-(kx + kw_));
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {                                  // sW[kh][n = kw*Cout+co][ci] (zero rows for n >= 9*Cout), once
        float wq[18];
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int e = tid + 256 * (18 * h + u), ci = e & 31, n = (e >> 5) & 31, kh = e >> 10;
            const int nn = n < NN ? n : 0, kw = nn / a.Cout, co = nn % a.Cout;
            const float v = a.w[(((size_t)kh * 9 + kw) * 32 + ci) * a.Cout + co];
            wq[u] = n < NN ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int e = tid + 256 * (18 * h + u), ci = e & 31, n = (e >> 5) & 31, kh = e >> 10;
            h16_t h0, h1;
            s9_split(wq[u], sw, h0, h1);
            const int o = (kh * 32 + n) * 32 + 8 * ((ci >> 3) ^ ((n >> 2) & 3)) + (ci & 7);
            sW0[o] = h0;
            sW1[o] = h1;
        }
    }
    // staging: piece tid + 256 u = the eight channels 8 half .. 8 half + 7 of the chunk at pixel (row wv + 4 u, column pcol)
    const int pcol = (tid >> 1) & 31, half = tid & 1;
    const int frel = ((wv - 4) * a.W + (pcol - 4)) * 32 + 8 * half;           // floats from the tile's origin pixel (y0, x0), u = 0
    const int fdst = (wv * S9G_TQ + pcol) * 16 + 8 * (half ^ ((pcol >> 3) & 1));
    u32x4_t vin[8];
    auto origin = [&](int tile, int& b, int& x0, int& y0) {
        b = tile / (tiles_x * tiles_y);
        const int tt = tile - b * (tiles_x * tiles_y);
        x0 = (tt % tiles_x) * S9G_TWO;
        y0 = (tt / tiles_x) * S9_TH;
    };
    auto fetch = [&](int tile, int c0) {
        int b, x0, y0;
        origin(tile, b, x0, y0);
        const BufRsrc rx = dasr_make_rsrc(a.x + (size_t)b * a.H * a.W * 32, (size_t)a.H * a.W * 32 * sizeof(float));
        // (masks, not selects on a condition: hipcc turns `column ok && row ok ? .. : DASR_OOB` into branches around the loads)
        const unsigned cm = (unsigned)(x0 - 4 + pcol) < (unsigned)a.W ? 0u : ~0u;
        const int base = (y0 * a.W + x0) * 32 + c0 + frel;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned m = cm | ((unsigned)(y0 - 4 + wv + 4 * u) < (unsigned)a.H ? 0u : ~0u);
            const unsigned off = ((unsigned)((base + u * 4 * a.W * 32) * (int)sizeof(float)) & ~m) | (DASR_OOB & m);
            vin[2 * u] = dasr_buffer_load16(rx, off);
            vin[2 * u + 1] = dasr_buffer_load16(rx, off + 16);
        }
    };
    // the shift-add: output tid + 256 u = (tile row orow, column ocol, channel co) - from sP float ospo + kw (PST + Cout) on,
    // to float orel from the tile's origin pixel in y
    int orow[S9G_NOUT], ocol[S9G_NOUT], ospo[S9G_NOUT], orel[S9G_NOUT];
    float obias[S9G_NOUT];
#pragma unroll
    for (int u = 0; u < S9G_NOUT; ++u) {
        const int idx = tid + 256 * u;
        const bool in = idx < S9_TH * S9G_TWO * a.Cout;
        const int co = idx % a.Cout, ox = (idx / a.Cout) % S9G_TWO, r = in ? idx / (a.Cout * S9G_TWO) : 0;
        orow[u] = r;
        ocol[u] = in ? ox : (1 << 28);                             // (past the tile's outputs: never inside the image)
        ospo[u] = (r * S9G_TQ + ox) * S9G_PST + co;
        orel[u] = (r * a.W + ox) * a.Cout + co;
        obias[u] = a.bias ? a.bias[co] : 0.f;
    }
    const int pstep = S9G_PST + a.Cout;
    const int asw = (li >> 3) & 1, bsw = (li >> 2) & 3;
    const int ab = (2 * wv * S9G_TQ + li) * 16 + 8 * (lh ^ asw);   // this lane's piece of input row 2 wv; + 512 per row
    const int wb = li * 32;                                        // ... of kernel row n = li, kh = 0; + 1024 per kh
    // (tiles in linear order, tile = workgroup + 512 trips: the 8 x 8 tile blocks per XCD that correspond to the first form's
    // order measured 5 % slower here - this form is bound by its own chain, not by where the halo is re-read from)
    int tile = blockIdx.x;
    if (tile < total) fetch(tile, 0);
    for (; tile < total; tile += gridDim.x) {
        const int ntile = tile + (int)gridDim.x < total ? tile + (int)gridDim.x : tile;      // (past the end: re-reads this tile)
        int b, x0, y0;
        origin(tile, b, x0, y0);
        f32x16 acc[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            DASR_LDS_BARRIER();                            // every wave is done with the previous chunk / tile (incl. its P image)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float f[8];
                memcpy(f, &vin[2 * u], 16);
                memcpy(f + 4, &vin[2 * u + 1], 16);
                h16x8 p0, p1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    h16_t h0, h1;
                    s9_split(f[j], sx, h0, h1);
                    p0[j] = h0; p1[j] = h1;
                }
                *(h16x8*)(sIn0 + fdst + u * 4 * S9G_TQ * 16) = p0;
                *(h16x8*)(sIn1 + fdst + u * 4 * S9G_TQ * 16) = p1;
            }
            DASR_LDS_BARRIER();
            fetch(c == 1 ? ntile : tile, c == 1 ? 0 : 16);     // the next chunk of this tile, or the first chunk of the next tile
            {
                // kh step: the operands of step kh + 1 are read while step kh multiplies
                const int pw = 8 * ((2 * c + lh) ^ bsw);
                h16x8 A0 = *(const h16x8*)(sIn0 + ab), A1 = *(const h16x8*)(sIn1 + ab);
                h16x8 N0 = *(const h16x8*)(sIn0 + ab + 512), N1 = *(const h16x8*)(sIn1 + ab + 512);
                h16x8 B0 = *(const h16x8*)(sW0 + wb + pw), B1 = *(const h16x8*)(sW1 + wb + pw);
                DASR_SCHED_BARRIER();
#pragma unroll
                for (int kh = 0; kh < 9; ++kh) {
                    const h16x8 a0 = A0, a1 = A1, n0 = N0, n1 = N1, b0 = B0, b1 = B1;
                    A0 = n0; A1 = n1;
                    if (kh + 1 < 9) {
                        N0 = *(const h16x8*)(sIn0 + ab + (kh + 2) * 512); N1 = *(const h16x8*)(sIn1 + ab + (kh + 2) * 512);
                        B0 = *(const h16x8*)(sW0 + wb + (kh + 1) * 1024 + pw); B1 = *(const h16x8*)(sW1 + wb + (kh + 1) * 1024 + pw);
                    }
                    acc[0] = s9_mma(a0, a1, b0, b1, acc[0]);
                    acc[1] = s9_mma(n0, n1, b0, b1, acc[1]);
                    if (kh + 1 < 9) DASR_SCHED_GROUP(0x100, 4);    // (hipcc otherwise sinks the reads to just before their use)
                    DASR_SCHED_GROUP(0x8, 6);
                }
                DASR_SCHED_BARRIER();
            }
        }
        DASR_LDS_BARRIER();
        float* sP = (float*)smem;   // [8][32][PST]
        if (li < S9G_PST) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int qx = (g & 3) + 8 * (g >> 2) + 4 * lh;
                    sP[((2 * wv + m) * S9G_TQ + qx) * S9G_PST + li] = acc[m][g];
                }
        }
        DASR_LDS_BARRIER();
        const BufRsrc ry = dasr_make_rsrc((float*)a.out + (size_t)b * a.H * a.W * a.Cout, (size_t)a.H * a.W * a.Cout * sizeof(float));
        const int obase = (y0 * a.W + x0) * a.Cout;
#pragma unroll
        for (int u = 0; u < S9G_NOUT; ++u) {
            const bool ok = y0 + orow[u] < a.H && x0 + ocol[u] < a.W;
            float v = 0.f;
#pragma unroll
            for (int kw = 0; kw < 9; ++kw) v += sP[ospo[u] + kw * pstep];
            dasr_buffer_store4f(ry, ok ? (unsigned)((obase + orel[u]) * (int)sizeof(float)) : DASR_OOB, fmaf(v, inv, obias[u]));
        }
    }
}

// ------------------------------------------------------------------------------------------ the E image (dgrad / wgrad)
// E[row][px][k'] (two fp16 images) = sd * dy row image [Cout*px + k'], 0 for k' >= 9 Cout, the dy tile's rows y0-4 .. y0+11 with
// Cout channels interleaved (zero outside the image).  Every dy value is scaled and split ONCE into two fp16 row images; a
// 16-byte piece of E (row, px, 8 k') is eight consecutive fp16 of a row from any element offset: five aligned dwords and
// v_alignbit_b32.  The wgrad's tile is 8 rows x 32 columns (below), the dgrad's 8 x 16.
#define S9_TQ 32
#define S9_DYW ((S9_TQ + 8) * 3 + 8)      // wgrad dy tile row stride: 40 px * 3 ch + pad = 128
constexpr int S9_NDYE = (S9_TH + 8) * S9_DYW, S9_NDI = S9_NDYE / 512;
static_assert(S9_NDI * 512 == S9_NDYE && S9_DYW == 128, "dy tile: whole trips of 512 threads, four threads' elements one column");

// ------------------------------------------------------------------------------------------ dgrad
// 256 threads, TWO workgroups per CU (74.9 KB of LDS each) whose phases overlap: while one stages dy / builds its E image /
// stores, the other multiplies.  tile: 8 rows x 16 columns of dx pixels x 32 input channels (blockIdx.y selects the
// 32-channel slice); wave w owns tile rows 2w, 2w+1 as ONE 32-pixel M-tile, lane li = row li >> 4, column li & 15:
// 9 kh x 2 K-halves x 3 products = 54 MFMAs per wave and tile, the K order of every output element what it always was.
// With the accumulator map row = (reg&3) + 8(reg>>2) + 4(lane>>5), registers g and g + 8 hold image rows 2w and 2w+1 of one
// column, g&3 = 0,1 / 2,3 two even/odd column pairs: a lane owns the complete 2 x 2 blocks of its channel.
// FUSE: the producer's activation / PixelShuffle(2) backward in the epilogue - x_act = this convolution's saved input (the
// producer's post-activation, shuffled output), dprev[b][y/2][x/2][4c + 2(y&1) + (x&1)] = dx[b][y][x][c] * act'(x_act): one
// float4 per 2 x 2 block, the 32 channel lanes of a half-wave write 512 contiguous bytes - and max |dprev| for the
// producer's own gradients (amax buffer, one word per workgroup).
// LDS: E as 2 x [16 rows][16 px][32 k'] and Wd as 2 x [9 kh][32 ci][32 k'] fp16, 64-byte pixel / channel stride with the
// 16-byte piece index XORed with (px >> 2) & 3 resp. (ci >> 2) & 3: each 16-lane group of a ds_read_b128 (MI355X: lanes
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of a half-wave) meets the pieces 0..3 of every bank quarter once.
// Global stores and the x_act loads go through range-checked buffer descriptors (ragged tiles: DASR_OOB, dropped), so every
// wave issues the same number of vector-memory operations per tile and the barriers are LDS-only: stores drain under the
// next tile's work instead of at its first barrier.
#define S9D_TQ 16
#define S9D_DYW ((S9D_TQ + 8) * 3 + 8)    // dy tile row stride: 24 px * 3 ch + pad = 80 (E pieces read up to element 3*15 + 31 + 2)
constexpr int S9D_NDYE = (S9_TH + 8) * S9D_DYW, S9D_NDI = S9D_NDYE / 256;
static_assert(S9D_NDI * 256 == S9D_NDYE, "dy tile: whole trips of 256 threads");
constexpr size_t S9D_LDS = sizeof(h16_t) * (size_t)(2 * (S9_TH + 8) * S9D_TQ * 32 + 2 * 9 * 32 * 32) + sizeof(float) * (size_t)(S9D_NDYE + 32);     // (the dy tile: two fp16 images)
static_assert(2 * S9D_LDS <= 160 * 1024, "two workgroups per CU");
typedef unsigned u32a_t __attribute__((may_alias));
typedef unsigned u32x4a_t __attribute__((ext_vector_type(4), may_alias));
// the low dword of {hi, lo} >> bits (bits = 0 or 16: eight fp16 from any element offset out of aligned dword reads)
__device__ __forceinline__ unsigned s9d_fsh(unsigned lo, unsigned hi, unsigned bits) {
#if DASR_DEVICE_BUILD
    return __builtin_amdgcn_alignbit(hi, lo, bits);
#else
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> bits);
#endif
}
template <bool FUSE>
__global__ void __launch_bounds__(256, 2) k_conv9_dgrad_split(Conv9SplitArgs a) {
    DASR_DYN_SMEM(smem);
    constexpr int NE = (S9_TH + 8) * S9D_TQ * 32;
    h16_t* sE0 = (h16_t*)smem;                                     // [16][16][32], pieces swizzled
    h16_t* sE1 = sE0 + NE;
    h16_t* sW0 = sE1 + NE;                                         // [9 kh][32 ci][32]: Wd[kh][k'][ci], k' contiguous, pieces swizzled
    h16_t* sW1 = sW0 + 9 * 32 * 32;
    h16_t* sH0 = sW1 + 9 * 32 * 32;                                // [16][DYW]: the dy tile, split ONCE per value
    h16_t* sH1 = sH0 + S9D_NDYE;
    float* s_red = (float*)(sH1 + S9D_NDYE);                       // [32]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int tiles_x = (a.W + S9D_TQ - 1) / S9D_TQ, tiles_y = (a.H + S9_TH - 1) / S9_TH;
    const int total = tiles_x * tiles_y * a.B;
    const int n0 = blockIdx.y * 32;
    const int KK = 9 * a.Cout;
    int kd, kw_;
    s9_scales(a.dmax, a.wmax, s_red, kd, kw_);
    const float sd = s9_pow2(kd), sw = s9_pow2(kw_), inv = s9_pow2(-(kd + kw_));
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {                                  // Wd[kh][k'][ci] = w[kh][8 - k'/Cout][ci][k' % Cout], once
        float wq[18];
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int e = tid + 256 * (18 * h + u), kp = e & 31, ci = (e >> 5) & 31, kh = e >> 10;
            const int kq = kp < KK ? kp : 0, kw = 8 - kq / a.Cout, co = kq % a.Cout;
            const float v = a.w[(((size_t)kh * 9 + kw) * a.Cin + n0 + ci) * a.Cout + co];
            wq[u] = kp < KK ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 18; ++u) {
            const int e = tid + 256 * (18 * h + u), kp = e & 31, ci = (e >> 5) & 31, kh = e >> 10;
            h16_t h0, h1;
            s9_split(wq[u], sw, h0, h1);
            const int o = (kh * 32 + ci) * 32 + 8 * ((kp >> 3) ^ ((ci >> 2) & 3)) + (kp & 7);
            sW0[o] = h0;
            sW1[o] = h1;
        }
    }
    // dy tile, rows y0-4 .. y0+11, columns x0-4 .. x0+19, Cout channels interleaved: element tid + 256 u is float f of tile row
    // ry - what does not depend on the tile is worked out once (the divisions by Cout above all)
    int dyr[S9D_NDI], dyx[S9D_NDI], dyo[S9D_NDI];
#pragma unroll
    for (int u = 0; u < S9D_NDI; ++u) {
        const int idx = tid + 256 * u, f = idx % S9D_DYW, ry = idx / S9D_DYW;
        dyr[u] = ry - 4;
        dyx[u] = f < (S9D_TQ + 8) * a.Cout ? f / a.Cout - 4 : (1 << 28);       // (the row's padding: never inside the image)
        dyo[u] = (dyr[u] * a.W - 4) * a.Cout + f;                             // floats from the tile's origin pixel (y0, x0)
    }
    float vdy[S9D_NDI];
    auto origin = [&](int tile, int& b, int& x0, int& y0) {
        b = tile / (tiles_x * tiles_y);
        const int tt = tile - b * (tiles_x * tiles_y);
        x0 = (tt % tiles_x) * S9D_TQ;
        y0 = (tt / tiles_x) * S9_TH;
    };
    // the next tile's dy values stay in flight in registers (zero outside the image: the descriptor's range check)
    auto fetch = [&](int b, int y0, int x0) {
        const BufRsrc rd = dasr_make_rsrc(a.dy + (size_t)b * a.H * a.W * a.Cout, (size_t)a.H * a.W * a.Cout * sizeof(float));
        const int base = (y0 * a.W + x0) * a.Cout;
#pragma unroll
        for (int u = 0; u < S9D_NDI; ++u) {
            const bool ok = (unsigned)(y0 + dyr[u]) < (unsigned)a.H && (unsigned)(x0 + dyx[u]) < (unsigned)a.W;
            vdy[u] = dasr_buffer_load4f(rd, ok ? (unsigned)((base + dyo[u]) * (int)sizeof(float)) : DASR_OOB);
        }
    };
    const int prow = 2 * wv + (li >> 4), pcol = li & 15;            // this lane's pixel as the A operand's row
    const int asw = (pcol >> 2) & 3, bsw = (li >> 2) & 3;
    // E[row][px][k'] = dy row image [Cout px + k'] (0 for k' >= 9 Cout), 16-byte pieces (row, px, 8 k'): this thread builds
    // the piece (px, p8) of rows r0, r0 + 4, .. - eight fp16 from element es of the row, any parity, out of five aligned dwords
    const int p8 = tid & 3, epx = (tid >> 2) & 15, r0 = tid >> 6;
    const int es = a.Cout * epx + 8 * p8;
    const unsigned ebits = (es & 1) * 16;
    const int esrc = r0 * S9D_DYW + (es & ~1), edst = (r0 * S9D_TQ + epx) * 32 + 8 * (p8 ^ ((epx >> 2) & 3));
    unsigned em[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) em[d] = (8 * p8 + 2 * d < KK ? 0xffffu : 0u) | (8 * p8 + 2 * d + 1 < KK ? 0xffff0000u : 0u);
    const size_t img = (size_t)a.H * a.W * a.Cin;                  // floats per sample of dx, x_act and dprev alike
    const unsigned rowst = (unsigned)(a.W * a.Cin) * sizeof(float), pixst = (unsigned)a.Cin * sizeof(float);
    // dasr_act_grad_from_out(v, act) = v > 0 ? 1 : dneg for the three activations the entry point admits
    const float dneg = a.act == DASR_ACT_RELU ? 0.f : (a.act == DASR_ACT_LRELU02 ? 0.2f : 1.f);
    float om = 0.f;
    int tile = blockIdx.x;
    if (tile < total) {
        int b, x0, y0;
        origin(tile, b, x0, y0);
        fetch(b, y0, x0);
    }
    for (; tile < total; tile += gridDim.x) {
        int b, x0, y0;
        origin(tile, b, x0, y0);
        // (no barrier here: the row images were last read before the previous tile's second barrier, and E is written after this
        // tile's first)
#pragma unroll
        for (int u = 0; u < S9D_NDI; ++u) {
            h16_t h0, h1;
            s9_split(vdy[u], sd, h0, h1);
            sH0[tid + 256 * u] = h0;
            sH1[tid + 256 * u] = h1;
        }
        DASR_LDS_BARRIER();                                        // ... which every wave reaches after its K loop over E
        {
            int nb, nx0, ny0;
            origin(tile + (int)gridDim.x < total ? tile + (int)gridDim.x : tile, nb, nx0, ny0);
            fetch(nb, ny0, nx0);
        }
        // byte offsets of this lane's pixels in dx / x_act (one layout): column pairs 4 lh + {0, 2, 8, 10} of image row
        // y0 + 2 wv; + pixst: the odd column, + rowst: the row below (fused form, H and W even: a 2 x 2 block is inside or outside
        // as a whole; DASR_OOB + those stays out of range)
        unsigned xoff[4];
        const bool rowok = y0 + 2 * wv < a.H;
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) {
            const int cx = x0 + 4 * lh + 2 * (cp & 1) + 8 * (cp >> 1);
            xoff[cp] = (rowok && cx < a.W) ? (unsigned)((((y0 + 2 * wv) * a.W + cx) * a.Cin + n0 + li) * (int)sizeof(float)) : DASR_OOB;
        }
        auto pix_off = [&](int g) {      // accumulator register g: image row (g >> 3), column (g & 3) + 8 ((g >> 2) & 1) + 4 lh
            const unsigned o = xoff[((g >> 2) & 1) * 2 + ((g & 3) >> 1)] + (g >> 3) * rowst + (g & 1) * pixst;
            if (FUSE) return o;
            // (the plain form takes odd H and W: the lower row / the odd column can be outside on its own)
            return (y0 + 2 * wv + (g >> 3) < a.H && x0 + 4 * lh + (g & 3) + 8 * ((g >> 2) & 1) < a.W) ? o : DASR_OOB;
        };
        float xa[16];
        if (FUSE) {                                                // in flight across the E build and the K loop
            const BufRsrc rx = dasr_make_rsrc(a.xact + (size_t)b * img, img * sizeof(float));
#pragma unroll
            for (int g = 0; g < 16; ++g) xa[g] = dasr_buffer_load4f(rx, pix_off(g));
        }
#pragma unroll
        for (int i = 0; i < (S9_TH + 8) / 4; ++i) {
            const u32a_t* s0 = (const u32a_t*)(sH0 + esrc + i * 4 * S9D_DYW);
            const u32a_t* s1 = (const u32a_t*)(sH1 + esrc + i * 4 * S9D_DYW);
            u32x4_t o0, o1;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                o0[d] = s9d_fsh(s0[d], s0[d + 1], ebits) & em[d];
                o1[d] = s9d_fsh(s1[d], s1[d + 1], ebits) & em[d];
            }
            *(u32x4a_t*)(sE0 + edst + i * 4 * S9D_TQ * 32) = o0;
            *(u32x4a_t*)(sE1 + edst + i * 4 * S9D_TQ * 32) = o1;
        }
        DASR_LDS_BARRIER();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            // step s = (kh, K-half q): the operands of step s + 1 are read while step s multiplies
            // dy row of output row prow for this kh: prow - kh + 4 (+4 for the tile's first row y0-4) = prow - kh + 8
            const int wb = li * 32, eb = ((prow + 8) * S9D_TQ + pcol) * 32;
            const int pw0 = 8 * (lh ^ bsw), pw1 = 8 * ((2 + lh) ^ bsw), pe0 = 8 * (lh ^ asw), pe1 = 8 * ((2 + lh) ^ asw);
            h16x8 A0 = *(const h16x8*)(sE0 + eb + pe0), A1 = *(const h16x8*)(sE1 + eb + pe0);
            h16x8 B0 = *(const h16x8*)(sW0 + wb + pw0), B1 = *(const h16x8*)(sW1 + wb + pw0);
            DASR_SCHED_BARRIER();
#pragma unroll
            for (int s = 0; s < 18; ++s) {
                const h16x8 a0 = A0, a1 = A1, b0 = B0, b1 = B1;
                if (s + 1 < 18) {
                    const int kh = (s + 1) >> 1, q = (s + 1) & 1;
                    const int wo = wb + kh * 32 * 32 + (q ? pw1 : pw0), eo = eb - kh * S9D_TQ * 32 + (q ? pe1 : pe0);
                    A0 = *(const h16x8*)(sE0 + eo); A1 = *(const h16x8*)(sE1 + eo);
                    B0 = *(const h16x8*)(sW0 + wo); B1 = *(const h16x8*)(sW1 + wo);
                }
                acc = s9_mma(a0, a1, b0, b1, acc);
                if (s + 1 < 18) DASR_SCHED_GROUP(0x100, 4);        // (hipcc otherwise sinks the reads to just before their use)
                DASR_SCHED_GROUP(0x8, 3);
            }
            DASR_SCHED_BARRIER();                                  // (... and hoists the epilogue's use of x_act into the loop)
        }
        if (FUSE) {
            const BufRsrc rp = dasr_make_rsrc((float*)a.out + (size_t)b * img, img * sizeof(float));
            const int Wc = a.W >> 1, cy = (y0 >> 1) + wv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = 2 * (j & 1) + 4 * (j >> 1);          // 0, 2, 4, 6: column pair j, image rows 2 wv (g, g + 1) and 2 wv + 1 (g + 8, g + 9)
                const int cx = x0 + 4 * lh + 2 * (j & 1) + 8 * (j >> 1);
                const bool ok = xoff[j] != DASR_OOB;
                float4 o;
                o.x = acc[g] * inv * (xa[g] > 0.f ? 1.f : dneg);
                o.y = acc[g + 1] * inv * (xa[g + 1] > 0.f ? 1.f : dneg);
                o.z = acc[g + 8] * inv * (xa[g + 8] > 0.f ? 1.f : dneg);
                o.w = acc[g + 9] * inv * (xa[g + 9] > 0.f ? 1.f : dneg);
                dasr_buffer_store16f(rp, ok ? (unsigned)(((cy * Wc + (cx >> 1)) * (4 * a.Cin) + 4 * (n0 + li)) * (int)sizeof(float)) : DASR_OOB, o);
                om = fmaxf(om, ok ? dasr_amax4(0.f, o) : 0.f);
            }
        } else {
            const BufRsrc ro = dasr_make_rsrc((float*)a.out + (size_t)b * img, img * sizeof(float));
            if (a.accumulate) {
                float old[16];
#pragma unroll
                for (int g = 0; g < 16; ++g) old[g] = dasr_buffer_load4f(ro, pix_off(g));
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    float v = acc[g] * inv;
                    v += old[g];
                    dasr_buffer_store4f(ro, pix_off(g), v);
                }
            } else {
#pragma unroll
                for (int g = 0; g < 16; ++g) dasr_buffer_store4f(ro, pix_off(g), acc[g] * inv);
            }
        }
    }
    // every thread of every workgroup arrives (the grid never exceeds the tile count: no workgroup is idle)
    if (FUSE && a.amax) dasr_amax_commit(a.amax, om, s_red, dasr_flat_wg(), dasr_flat_nwg());
}

// ------------------------------------------------------------------------------------------ wgrad
// blockIdx.x = 32-channel slice of Cin, blockIdx.y = partial index p (tiles p, p+P, ...).  512 threads: wave w owns
// tile row w, all nine kh (9 accumulators = dW[kh] as a 32 ci x 32 k' tile).  K = pixels, so both operands are read
// TRANSPOSED from pixel-major LDS tiles with ds_read_b64_tr_b16 (on 16-bit fp16 elements): A = x^T ([ci][pixel]),
// B = E^T.  Each wave writes its own slab [9][32][32] (times the inverse of the two scales); k_conv9_wgrad_reduce_split
// sums the slabs and un-folds k'.  The dy tile is split once into two fp16 row images and E built from them (see above: the
// piece (px, 8 k') of rows r0, r0 + 4, .. per thread); the loads go through range-checked descriptors with what does not
// depend on the tile worked out once, and the barriers are LDS-only: the next tile's loads stay in flight across the E
// build AND the MFMA phase.
__device__ __forceinline__ h16x4 s9_read_tr16(const h16_t* p) {
    const bf16x4 r = lds_read_tr16((const bf16_t*)p);
    h16x4 v;
    __builtin_memcpy(&v, &r, 8);
    return v;
}
__global__ void __launch_bounds__(512) k_conv9_wgrad_split(Conv9SplitArgs a) {
    DASR_DYN_SMEM(smem);
    constexpr int EST = 32;                                        // 64-byte pixel stride: conflict-free transposed reads
    constexpr int NX = S9_TH * S9_TQ * 32, NE = (S9_TH + 8) * S9_TQ * EST;
    h16_t* sX0 = (h16_t*)smem;                                     // [8][32][32]
    h16_t* sX1 = sX0 + NX;
    h16_t* sE0 = sX1 + NX;                                         // [16][32][EST]
    h16_t* sE1 = sE0 + NE;
    h16_t* sH0 = sE1 + NE;                                         // [16][DYW]: the dy tile, split ONCE per value
    h16_t* sH1 = sH0 + S9_NDYE;
    float* s_red = (float*)(sH1 + S9_NDYE);                        // [32]
    const int tid = threadIdx.x, lane = tid & 63, wv = DASR_UNIFORM((int)(tid >> 6)), li = lane & 31, lh = lane >> 5;
    const int tiles_x = (a.W + S9_TQ - 1) / S9_TQ, tiles_y = (a.H + S9_TH - 1) / S9_TH;
    const int ci0 = blockIdx.x * 32;
    int kx, kd;
    s9_scales(a.xmax, a.dmax, s_red, kx, kd);
    const float sx = s9_pow2(kx), sd = s9_pow2(kd), inv = s9_pow2(-(kx + kd));
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;
    constexpr int NXP = S9_TH * S9_TQ * 8 / 512;                   // 4 pieces of 16 bytes (4 channels) per thread
    u32x4_t vx[NXP];
    float vdy[S9_NDI];
    // dy tile, rows y0-4 .. y0+11, columns x0-4 .. x0+35, Cout channels interleaved: element tid + 512 u is float f = tid & 127
    // of tile row r0 + 4 u - the column and the division by Cout are the same for every u and every tile
    const int KK = 9 * a.Cout;
    const int r0 = DASR_UNIFORM((int)(tid >> 7)), dyf = tid & (S9_DYW - 1);
    const int dyx = dyf < (S9_TQ + 8) * a.Cout ? dyf / a.Cout - 4 : (1 << 28);       // (the row's padding: never inside the image)
    const int dyo = ((r0 - 4) * a.W - 4) * a.Cout + dyf;                             // floats from the tile's origin pixel (y0, x0), u = 0
    // E: this thread builds the piece (px, p8) of rows r0, r0 + 4, .. - eight fp16 from element es of the row, any parity
    const int p8 = tid & 3, epx = (tid >> 2) & 31;
    const int es = a.Cout * epx + 8 * p8;
    const unsigned ebits = (es & 1) * 16;
    const int esrc = r0 * S9_DYW + (es & ~1), edst = (r0 * S9_TQ + epx) * EST + 8 * p8;
    unsigned em[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) em[d] = (8 * p8 + 2 * d < KK ? 0xffffu : 0u) | (8 * p8 + 2 * d + 1 < KK ? 0xffff0000u : 0u);
    auto origin = [&](int tile, int& b, int& x0, int& y0) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y;
        b = tile / (tiles_x * tiles_y);
        x0 = tx * S9_TQ;
        y0 = ty * S9_TH;
    };
    auto fetch = [&](int tile) {
        int b, x0, y0;
        origin(tile, b, x0, y0);
        const BufRsrc rx = dasr_make_rsrc(a.x + (size_t)b * a.H * a.W * a.Cin, (size_t)a.H * a.W * a.Cin * sizeof(float));
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 512 * u, pix = idx >> 3, q8 = idx & 7;
            const int gy = y0 + pix / S9_TQ, gx = x0 + pix % S9_TQ;
            vx[u] = dasr_buffer_load16(rx, (gy < a.H && gx < a.W)
                                               ? (unsigned)(((gy * a.W + gx) * a.Cin + ci0 + 4 * q8) * (int)sizeof(float))
                                               : DASR_OOB);
        }
        // (zero outside the image: the descriptor's range check; masks, not selects, so that hipcc does not branch around loads)
        const BufRsrc rd = dasr_make_rsrc(a.dy + (size_t)b * a.H * a.W * a.Cout, (size_t)a.H * a.W * a.Cout * sizeof(float));
        const unsigned cm = (unsigned)(x0 + dyx) < (unsigned)a.W ? 0u : ~0u;
        const int base = (y0 * a.W + x0) * a.Cout + dyo;
#pragma unroll
        for (int u = 0; u < S9_NDI; ++u) {
            const unsigned m = cm | ((unsigned)(y0 + r0 - 4 + 4 * u) < (unsigned)a.H ? 0u : ~0u);
            vdy[u] = dasr_buffer_load4f(rd, ((unsigned)((base + 4 * u * a.W * a.Cout) * (int)sizeof(float)) & ~m) | (DASR_OOB & m));
        }
    };
    int tile = blockIdx.y;
    if (tile < a.ntiles) fetch(tile);
    for (; tile < a.ntiles; tile += a.P) {
        DASR_LDS_BARRIER();                      // every wave is done with the previous tile
#pragma unroll
        for (int u = 0; u < S9_NDI; ++u) {
            h16_t h0, h1;
            s9_split(vdy[u], sd, h0, h1);
            sH0[tid + 512 * u] = h0;
            sH1[tid + 512 * u] = h1;
        }
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 512 * u;
            float f[4];
            memcpy(f, &vx[u], 16);
            h16x4 p0, p1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h16_t h0, h1;
                s9_split(f[j], sx, h0, h1);
                p0[j] = h0; p1[j] = h1;
            }
            *(h16x4*)(sX0 + (idx >> 3) * 32 + 4 * (idx & 7)) = p0;
            *(h16x4*)(sX1 + (idx >> 3) * 32 + 4 * (idx & 7)) = p1;
        }
        DASR_LDS_BARRIER();
        fetch(tile + a.P < a.ntiles ? tile + a.P : tile);
#pragma unroll
        for (int i = 0; i < (S9_TH + 8) / 4; ++i) {
            const u32a_t* s0 = (const u32a_t*)(sH0 + esrc + i * 4 * S9_DYW);
            const u32a_t* s1 = (const u32a_t*)(sH1 + esrc + i * 4 * S9_DYW);
            u32x4_t o0, o1;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                o0[d] = s9d_fsh(s0[d], s0[d + 1], ebits) & em[d];
                o1[d] = s9d_fsh(s1[d], s1[d + 1], ebits) & em[d];
            }
            *(u32x4a_t*)(sE0 + edst + i * 4 * S9_TQ * EST) = o0;
            *(u32x4a_t*)(sE1 + edst + i * 4 * S9_TQ * EST) = o1;
        }
        DASR_LDS_BARRIER();
        // K-step = 16 consecutive pixels of this wave's row
#pragma unroll
        for (int s = 0; s < S9_TQ / 16; ++s) {
            const int px = 16 * s + 8 * lh + tq;
            const int xo = (wv * S9_TQ + px) * 32 + 16 * tg + 4 * tp;
            h16x8 a0, a1;
            {
                const h16x4 l0 = s9_read_tr16(sX0 + xo), u0 = s9_read_tr16(sX0 + xo + 4 * 32);
                const h16x4 l1 = s9_read_tr16(sX1 + xo), u1 = s9_read_tr16(sX1 + xo + 4 * 32);
#pragma unroll
                for (int e = 0; e < 4; ++e) { a0[e] = l0[e]; a0[4 + e] = u0[e]; a1[e] = l1[e]; a1[4 + e] = u1[e]; }
            }
#pragma unroll
            for (int kh = 0; kh < 9; ++kh) {
                const int eo = ((wv - kh + 8) * S9_TQ + px) * EST + 16 * tg + 4 * tp;
                const h16x4 l0 = s9_read_tr16(sE0 + eo), u0 = s9_read_tr16(sE0 + eo + 4 * EST);
                const h16x4 l1 = s9_read_tr16(sE1 + eo), u1 = s9_read_tr16(sE1 + eo + 4 * EST);
                h16x8 b0, b1;
#pragma unroll
                for (int e = 0; e < 4; ++e) { b0[e] = l0[e]; b0[4 + e] = u0[e]; b1[e] = l1[e]; b1[4 + e] = u1[e]; }
                acc[kh] = s9_mma(a0, a1, b0, b1, acc[kh]);
            }
        }
    }
    float* slab = (float*)a.out + ((size_t)(blockIdx.y * 8 + wv) * gridDim.x + blockIdx.x) * (9 * 32 * 32);
#pragma unroll
    for (int kh = 0; kh < 9; ++kh)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int ci = (g & 3) + 8 * (g >> 2) + 4 * lh;
            slab[(kh * 32 + ci) * 32 + li] = acc[kh][g] * inv;
        }
}

// dw[kh][kw][ci][co] = sum over slabs of slab[cig][kh][ci%32][(8-kw)*Cout+co], every element's slabs in a fixed order (bitwise
// repeatable from launch to launch, no atomics, nothing to clear beforehand).  A workgroup owns one slab row (cig, kh, ci % 32:
// 32 k', 128 contiguous bytes); its 16 thread groups sum the slabs q, q + 16, ... with eight loads in flight per thread (the
// slabs were just written: the latency chain, not the bytes, is what the launch waits for) and meet in LDS.
__global__ void __launch_bounds__(512) k_conv9_wgrad_reduce_split(const float* __restrict__ slabs, float* __restrict__ dw,
                                                                  int Cin, int Cout, int nslabs, int cgroups) {
    __shared__ float part[16][32];
    const int np = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int row = blockIdx.x, cl = row & 31, kh = (row >> 5) % 9, cig = row / (9 * 32);
    const bool in = np < 9 * Cout;
    float acc = 0.f;
    if (in) {
        const float* p = slabs + (size_t)cig * (9 * 32 * 32) + (kh * 32 + cl) * 32 + np;
        const size_t st = (size_t)cgroups * (9 * 32 * 32);
        for (int s0 = q; s0 < nslabs; s0 += 8 * 16) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s0 + 16 * u < nslabs ? p[(size_t)(s0 + 16 * u) * st] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
    }
    part[q][np] = acc;
    __syncthreads();
    if (q == 0 && in) {
        float r = part[0][np];
#pragma unroll
        for (int t = 1; t < 16; ++t) r += part[t][np];
        const int kw = 8 - np / Cout, co = np % Cout;
        dw[(((size_t)kh * 9 + kw) * Cin + cig * 32 + cl) * Cout + co] = r;
    }
}

// ------------------------------------------------------------------------------------------ host side
bool conv9_split_supported(const ConvGeom& g) {
    return conv9_mfma_supported(g) && (g.Cin / 16) * 9 * 32 * S9F_ST * 2 * 2 + (S9_TH + 8) * S9F_TQ * S9F_ST * 2 * 2 + 128 <= 160 * 1024 &&
           (size_t)g.H * g.W * g.Cin * sizeof(float) < ((size_t)1 << 31);
}
int conv9_split_fwd(const ConvGeom& g, const float* x, const float* xmax, const float* w, const float* wmax, const float* bias,
                    float* y, void* stream) {
    Conv9SplitArgs a{x, w, bias, nullptr, y, xmax, nullptr, wmax, g.B, g.H, g.W, g.Cin, g.Cout, 0, 0, 0};
    if (g.Cin == 32 && (dasr_get_conv_bf16_impl() & 8192) == 0) {      // (+ 8192: the first form, A/B and tests)
        const int tiles = ((g.W + S9G_TWO - 1) / S9G_TWO) * ((g.H + S9_TH - 1) / S9_TH) * g.B;
        const int cap = (dasr_get_conv_bf16_impl() & 3) == 2 ? 3 : 512;    // (impl 2, tests: long per-workgroup tile lists)
        DASR_LAUNCH(k_conv9_fwd_split, dim3(tiles < cap ? tiles : cap), dim3(256), S9G_LDS, stream, a);     // two persistent workgroups per CU
        DASR_RETURN_LAUNCH_STATUS();
    }
    const int TWO = S9F_TQ - 8;
    const int tiles = ((g.W + TWO - 1) / TWO) * ((g.H + S9_TH - 1) / S9_TH) * g.B;
    const size_t lds = sizeof(h16_t) * (size_t)(2 * (S9_TH + 8) * S9F_TQ * S9F_ST + 2 * (g.Cin / 16) * 9 * 32 * S9F_ST) + 128;
    const int cap = (dasr_get_conv_bf16_impl() & 3) == 2 ? 3 : 256;    // (impl 2, tests: long per-workgroup tile lists)
    a.P = (tiles >= 256 && cap == 256 && (dasr_get_conv_bf16_impl() & 4096) == 0) ? 1 : 0;      // XCD-blocked tile order (+ 4096: linear, A/B)
    DASR_LAUNCH(k_conv9_fwd_split_1wg, dim3(tiles < cap ? tiles : cap), dim3(512), lds, stream, a);     // one persistent workgroup per CU
    DASR_RETURN_LAUNCH_STATUS();
}
static int conv9_split_dgrad_launch(const ConvGeom& g, Conv9SplitArgs& a, bool fuse, void* stream) {
    const int tiles = ((g.W + S9D_TQ - 1) / S9D_TQ) * ((g.H + S9_TH - 1) / S9_TH) * g.B;
    int per = 512 / (g.Cin / 32) > 0 ? 512 / (g.Cin / 32) : 1;               // persistent: two workgroups per CU over all slices
    if ((dasr_get_conv_bf16_impl() & 3) == 2) per = 3;
    const dim3 grid(tiles < per ? tiles : per, g.Cin / 32);
    if (fuse)
        DASR_LAUNCH(k_conv9_dgrad_split<true>, grid, dim3(256), S9D_LDS, stream, a);
    else
        DASR_LAUNCH(k_conv9_dgrad_split<false>, grid, dim3(256), S9D_LDS, stream, a);
    DASR_RETURN_LAUNCH_STATUS();
}
int conv9_split_dgrad(const ConvGeom& g, const float* dconv, const float* dmax, const float* w, const float* wmax, float* dx,
                      int accumulate, void* stream) {
    Conv9SplitArgs a{nullptr, w, nullptr, dconv, dx, nullptr, dmax, wmax, g.B, g.H, g.W, g.Cin, g.Cout, accumulate, 0, 0};
    return conv9_split_dgrad_launch(g, a, false, stream);
}
int conv9_split_dgrad_act(const ConvGeom& g, const float* dconv, const float* dmax, const float* w, const float* wmax,
                          const float* x_act, float* dprev, float* amax, int act, void* stream) {
    Conv9SplitArgs a{nullptr, w, nullptr, dconv, dprev, nullptr, dmax, wmax, g.B, g.H, g.W, g.Cin, g.Cout, 0, 0, 0, x_act, amax, act};
    return conv9_split_dgrad_launch(g, a, true, stream);
}
static void conv9_split_wgrad_plan(const ConvGeom& g, int& ntiles, int& P) {
    ntiles = g.B * ((g.H + S9_TH - 1) / S9_TH) * ((g.W + S9_TQ - 1) / S9_TQ);
    P = 256 / (g.Cin / 32);
    if ((dasr_get_conv_bf16_impl() & 3) == 2) P = 3;
    if (P > ntiles) P = ntiles;
    if (P < 1) P = 1;
}
size_t conv9_split_wgrad_workspace(const ConvGeom& g) {
    const int ntiles = g.B * ((g.H + S9_TH - 1) / S9_TH) * ((g.W + S9_TQ - 1) / S9_TQ);
    int P = 256 / (g.Cin / 32);
    if (P > ntiles) P = ntiles;
    if (P < 1) P = 1;
    return sizeof(float) * (size_t)P * 8 * (g.Cin / 32) * 9 * 32 * 32;
}
int conv9_split_wgrad(const ConvGeom& g, const float* x, const float* xmax, const float* dconv, const float* dmax, float* dw,
                      void* workspace, void* stream) {
    int ntiles, P;
    conv9_split_wgrad_plan(g, ntiles, P);
    Conv9SplitArgs a{x, nullptr, nullptr, dconv, workspace, xmax, dmax, nullptr, g.B, g.H, g.W, g.Cin, g.Cout, 0, P, ntiles};
    const size_t lds = sizeof(h16_t) * (size_t)(2 * S9_TH * S9_TQ * 32 + 2 * (S9_TH + 8) * S9_TQ * 32) +
                       sizeof(float) * (size_t)(S9_NDYE + 32);
    DASR_LAUNCH(k_conv9_wgrad_split, dim3(g.Cin / 32, P), dim3(512), lds, stream, a);
    DASR_LAUNCH(k_conv9_wgrad_reduce_split, dim3((g.Cin / 32) * 9 * 32), dim3(512), 0, stream, (const float*)workspace, dw, g.Cin,
                g.Cout, P * 8, g.Cin / 32);
    DASR_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" int dasr_conv9_split_supported(int H, int W, int Cin, int Cout) {
    ConvGeom g{1, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    return (H > 0 && W > 0 && Cin > 0 && Cout > 0 && conv9_split_supported(g)) ? 1 : 0;
}
extern "C" int dasr_conv9_fwd_split2(const float* x, const float* xmax, const float* w_hwio, const float* wmax, const float* bias,
                                     float* y, int B, int H, int W, int Cin, int Cout, void* stream) {
    DASR_CHECK_PTR(x); DASR_CHECK_PTR(xmax); DASR_CHECK_PTR(w_hwio); DASR_CHECK_PTR(wmax); DASR_CHECK_PTR(y);
    DASR_CHECK_SHAPE(B > 0);
    if (!dasr_conv9_split_supported(H, W, Cin, Cout)) return DASR_E_UNSUPPORTED;
    ConvGeom g{B, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    return conv9_split_fwd(g, x, xmax, w_hwio, wmax, bias, y, stream);
}
extern "C" int dasr_conv9_dgrad_split2(const float* dconv, const float* dmax, const float* w_hwio, const float* wmax, float* dx,
                                       int accumulate, int B, int H, int W, int Cin, int Cout, void* stream) {
    DASR_CHECK_PTR(dconv); DASR_CHECK_PTR(dmax); DASR_CHECK_PTR(w_hwio); DASR_CHECK_PTR(wmax); DASR_CHECK_PTR(dx);
    DASR_CHECK_SHAPE(B > 0);
    if (!dasr_conv9_split_supported(H, W, Cin, Cout)) return DASR_E_UNSUPPORTED;
    ConvGeom g{B, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    return conv9_split_dgrad(g, dconv, dmax, w_hwio, wmax, dx, accumulate, stream);
}
extern "C" int dasr_conv9_dgrad_act_split2(const float* dconv, const float* dmax, const float* w_hwio, const float* wmax,
                                           const float* x_act, float* dprev, float* amax, int B, int H, int W, int Cin, int Cout,
                                           int act, int ps_r, void* stream) {
    DASR_CHECK_PTR(dconv); DASR_CHECK_PTR(dmax); DASR_CHECK_PTR(w_hwio); DASR_CHECK_PTR(wmax); DASR_CHECK_PTR(x_act); DASR_CHECK_PTR(dprev);
    DASR_CHECK_SHAPE(B > 0);
    if (ps_r != 2 || (H & 1) || (W & 1) || !(act == DASR_ACT_NONE || act == DASR_ACT_RELU || act == DASR_ACT_LRELU02) ||
        !dasr_conv9_split_supported(H, W, Cin, Cout))
        return DASR_E_UNSUPPORTED;
    ConvGeom g{B, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    return conv9_split_dgrad_act(g, dconv, dmax, w_hwio, wmax, x_act, dprev, amax, act, stream);
}
extern "C" size_t dasr_conv9_wgrad_split2_workspace(int B, int H, int W, int Cin, int Cout) {
    if (B <= 0 || !dasr_conv9_split_supported(H, W, Cin, Cout)) return 0;
    ConvGeom g{B, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    return conv9_split_wgrad_workspace(g);
}
extern "C" int dasr_conv9_wgrad_split2(const float* x, const float* xmax, const float* dconv, const float* dmax, float* dw_hwio,
                                       float* dbias, void* workspace, size_t workspace_bytes, int B, int H, int W, int Cin,
                                       int Cout, void* stream) {
    DASR_CHECK_PTR(x); DASR_CHECK_PTR(xmax); DASR_CHECK_PTR(dconv); DASR_CHECK_PTR(dmax); DASR_CHECK_PTR(dw_hwio);
    DASR_CHECK_PTR(workspace);
    DASR_CHECK_SHAPE(B > 0);
    if (!dasr_conv9_split_supported(H, W, Cin, Cout)) return DASR_E_UNSUPPORTED;
    if (workspace_bytes < dasr_conv9_wgrad_split2_workspace(B, H, W, Cin, Cout)) return DASR_E_WORKSPACE;
    ConvGeom g{B, H, W, Cin, H, W, Cout, 9, 9, 1, 4, 0};
    int rc = conv9_split_wgrad(g, x, xmax, dconv, dmax, dw_hwio, workspace, stream);
    if (rc) return rc;
    if (dbias) rc = conv_colsum(dconv, dbias, (size_t)B * H * W, Cout, stream);
    return rc;
}
