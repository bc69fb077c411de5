// metrics.hip — the four figures of the reference's test script (codes/test.py:97-152) from two uint8 images, in one pass:
//
//   dasr_image_metrics_u8   per frame of two uint8 [B,H,W,C] batches (C = 3: BGR; C = 1) inside a `crop`-pixel border:
//                             ssd      exact integer sum of (a - b)^2, all channels        calculate_psnr, utils/util.py:646-653
//                             sums[0]  sum of (Ya - Yb)^2 of the BT.601 luma                bgr2ycbcr, data/util.py:199-213
//                             sums[1]  sum of the SSIM map over positions and channels      ssim / calculate_ssim,
//                             sums[2]  sum of the SSIM map of the luma image                utils/util.py:656-697
//
// SSIM here is the "same as MATLAB" form: a VALID 11 x 11 Gaussian window (sigma 1.5), constants on the [0, 255] scale, float64.
// It is not the number of ssim.hip (pytorch_ssim: zero padding, fp32, [0, 1] tensors).  Everything is fp64: E[x^2] - mu^2
// cancels at magnitude 65025 against C2 = 58.5, which fp32 cannot carry to the six decimals the script prints.
//
// A workgroup owns a MT_H x MT_W tile of the SSIM map.  It stages the (MT_H + 10) x (MT_W + 10) pixels under it as bytes in
// LDS once, then takes the planes one after the other (B, G, R, luma; or the single gray plane): plane values as doubles into
// LDS, an 11-tap row pass of the five moments into LDS, an 11-tap column pass into registers, the SSIM ratio, a sum.  The
// pixel sums (ssd, luma) run over the pixels a tile owns: its MT_H x MT_W corner, and for the last tile row / column the ten
// further rows / columns as well, so that the tiles partition the cropped image.  No atomics: every workgroup writes its
// four partials into its own words of the caller's workspace and a second launch adds the partials of a frame in index
// order - a frame's result has the same bits in every run and in every batch.
#include "dasr_common.h"

#define MT_H 16
#define MT_W 32
#define MT_R 5
#define MT_HH (MT_H + 2 * MT_R)         // 26 halo rows
#define MT_HW (MT_W + 2 * MT_R)         // 42 halo columns

struct MetricsArgs {
    const unsigned char* a;
    const unsigned char* b;
    unsigned long long* part_ssd;        // [B][tiles]
    double* part;                        // [B][tiles][3]
    int H, W, C, crop, Hc, Wc, tiles_x, tiles_y;
    double g[11];                        // exp(-(i-5)^2 / (2 * 1.5^2)), normalised to sum 1 in float64
};

__device__ __forceinline__ int metrics_min(int a, int b) { return a < b ? a : b; }

// bgr2ycbcr(only_y=True) of a float image, back on the [0, 255] scale, not rounded (data/util.py:205)
__device__ __forceinline__ double metrics_luma(unsigned b, unsigned g, unsigned r) {
    return fma(65.481, (double)r, fma(128.553, (double)g, 24.966 * (double)b)) / 255.0 + 16.0;
}

__device__ __forceinline__ double metrics_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                              // (red is reused from one sum to the next)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);                 // every thread holds the sum
}

__global__ void __launch_bounds__(256) k_image_metrics(MetricsArgs s) {
    __shared__ unsigned char sA8[MT_HH][MT_HW * 3], sB8[MT_HH][MT_HW * 3];
    __shared__ double sX[MT_HH][MT_HW], sY[MT_HH][MT_HW];
    __shared__ double sHz[5][MT_HH][MT_W];
    __shared__ double red[4];
    __shared__ unsigned long long red_u[4];
    const int tid = threadIdx.x, f = blockIdx.y, C = s.C;
    const int tile = blockIdx.x, tx = tile % s.tiles_x, ty = tile / s.tiles_x;
    const int y0 = ty * MT_H, x0 = tx * MT_W;                     // in the cropped image = in the SSIM map
    const int rows = metrics_min(MT_HH, s.Hc - y0), cols = metrics_min(MT_HW, s.Wc - x0);        // pixels of the halo that exist (>= 11)
    const int rowlen = cols * C;

    // ---- the bytes under the tile ----
    for (int i = tid; i < rows * rowlen; i += 256) {
        const int r = i / rowlen, e = i - r * rowlen;
        const size_t off = (((size_t)f * s.H + (s.crop + y0 + r)) * s.W + (s.crop + x0)) * C + e;
        sA8[r][e] = s.a[off];
        sB8[r][e] = s.b[off];
    }
    __syncthreads();

    // ---- the pixel sums over the pixels this tile owns ----
    const int own_r = ty == s.tiles_y - 1 ? rows : MT_H, own_c = tx == s.tiles_x - 1 ? cols : MT_W;
    unsigned long long ssd = 0;
    double ysd = 0.0;
    for (int i = tid; i < own_r * own_c; i += 256) {
        const int r = i / own_c, c = i - r * own_c;
        if (C == 3) {
            const unsigned ab = sA8[r][3 * c], ag = sA8[r][3 * c + 1], ar = sA8[r][3 * c + 2];
            const unsigned bb = sB8[r][3 * c], bg = sB8[r][3 * c + 1], br = sB8[r][3 * c + 2];
            const int d0 = (int)ab - (int)bb, d1 = (int)ag - (int)bg, d2 = (int)ar - (int)br;
            ssd += (unsigned)(d0 * d0 + d1 * d1 + d2 * d2);
            const double d = metrics_luma(ab, ag, ar) - metrics_luma(bb, bg, br);
            ysd = fma(d, d, ysd);
        } else {
            const int d = (int)sA8[r][c] - (int)sB8[r][c];
            ssd += (unsigned)(d * d);
        }
    }

    // ---- the SSIM map, plane by plane ----
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const int out_r = metrics_min(MT_H, rows - 2 * MT_R), out_c = metrics_min(MT_W, cols - 2 * MT_R);      // map positions of this tile
    const int planes = C == 3 ? 4 : 1;
    double acc_c = 0.0, acc_y = 0.0;
    for (int p = 0; p < planes; ++p) {
        __syncthreads();                                          // the previous plane's column pass has read sHz
        for (int i = tid; i < rows * cols; i += 256) {
            const int r = i / cols, c = i - r * cols;
            double va, vb;
            if (p < 3) {
                va = (double)sA8[r][C * c + p];
                vb = (double)sB8[r][C * c + p];
            } else {
                va = metrics_luma(sA8[r][3 * c], sA8[r][3 * c + 1], sA8[r][3 * c + 2]);
                vb = metrics_luma(sB8[r][3 * c], sB8[r][3 * c + 1], sB8[r][3 * c + 2]);
            }
            sX[r][c] = va;
            sY[r][c] = vb;
        }
        __syncthreads();
        // row pass: rows x out_c x 5 moments
        for (int i = tid; i < rows * out_c; i += 256) {
            const int r = i / out_c, c = i - r * out_c;
            double m1 = 0.0, m2 = 0.0, q11 = 0.0, q22 = 0.0, q12 = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double av = sX[r][c + k], bv = sY[r][c + k], w = s.g[k];
                m1 = fma(w, av, m1);
                m2 = fma(w, bv, m2);
                q11 = fma(w, av * av, q11);
                q22 = fma(w, bv * bv, q22);
                q12 = fma(w, av * bv, q12);
            }
            sHz[0][r][c] = m1; sHz[1][r][c] = m2; sHz[2][r][c] = q11; sHz[3][r][c] = q22; sHz[4][r][c] = q12;
        }
        __syncthreads();
        // column pass and the ratio (utils/util.py:665-675)
        double acc = 0.0;
        for (int i = tid; i < out_r * out_c; i += 256) {
            const int r = i / out_c, c = i - r * out_c;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double w = s.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fma(w, sHz[q][r + k][c], m[q]);
            }
            const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu12 = m[0] * m[1];
            const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
            acc += ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        }
        if (p < 3) acc_c += acc; else acc_y = acc;
    }

    // ---- one set of partials per workgroup ----
    for (int o = 32; o > 0; o >>= 1) ssd += __shfl_down(ssd, o, 64);
    if ((tid & 63) == 0) red_u[tid >> 6] = ssd;
    const double t_ysd = metrics_block_sum(ysd, red);
    const double t_c = metrics_block_sum(acc_c, red);
    const double t_y = metrics_block_sum(acc_y, red);
    if (tid == 0) {
        const size_t w = (size_t)f * gridDim.x + tile;
        s.part_ssd[w] = (red_u[0] + red_u[1]) + (red_u[2] + red_u[3]);
        s.part[3 * w] = t_ysd;
        s.part[3 * w + 1] = t_c;
        s.part[3 * w + 2] = t_y;
    }
}

// one workgroup per frame: thread t adds partials t, t + 256, ... in that order, then a fixed tree
__global__ void __launch_bounds__(256) k_image_metrics_final(const unsigned long long* __restrict__ part_ssd,
                                                             const double* __restrict__ part,
                                                             unsigned long long* __restrict__ ssd, double* __restrict__ sums,
                                                             int tiles) {
    __shared__ double red[3][256];
    __shared__ unsigned long long red_u[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    unsigned long long u = 0;
    double v[3] = {0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += 256) {
        const size_t w = (size_t)f * tiles + t;
        u += part_ssd[w];
        for (int q = 0; q < 3; ++q) v[q] += part[3 * w + q];
    }
    red_u[tid] = u;
    for (int q = 0; q < 3; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red_u[tid] += red_u[tid + o];
            for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ssd[f] = red_u[0];
        for (int q = 0; q < 3; ++q) sums[3 * (size_t)f + q] = red[q][0];
    }
}

// 0: refused.  The tiles of one frame.
static long long metrics_tiles(int B, int H, int W, int C, int crop, int* tiles_x, int* tiles_y) {
    if (B <= 0 || H <= 0 || W <= 0 || crop < 0 || (C != 1 && C != 3)) return 0;
    const long long Hc = (long long)H - 2 * (long long)crop, Wc = (long long)W - 2 * (long long)crop;
    if (Hc < 11 || Wc < 11) return 0;
    const long long ty = (Hc - 10 + MT_H - 1) / MT_H, tx = (Wc - 10 + MT_W - 1) / MT_W;
    if (tiles_x) *tiles_x = (int)tx;
    if (tiles_y) *tiles_y = (int)ty;
    return tx * ty;
}

extern "C" size_t dasr_image_metrics_u8_workspace(int B, int H, int W, int C, int crop) {
    const long long tiles = metrics_tiles(B, H, W, C, crop, nullptr, nullptr);
    return (size_t)tiles * (size_t)B * (sizeof(unsigned long long) + 3 * sizeof(double));
}

extern "C" int dasr_image_metrics_u8(const unsigned char* a, const unsigned char* b, unsigned long long* ssd, double* sums,
                                     void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int crop,
                                     void* stream) {
    DASR_CHECK_PTR(a); DASR_CHECK_PTR(b); DASR_CHECK_PTR(ssd); DASR_CHECK_PTR(sums); DASR_CHECK_PTR(workspace);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && C > 0 && crop >= 0 && B <= 65535);
    MetricsArgs s;
    const long long tiles = metrics_tiles(B, H, W, C, crop, &s.tiles_x, &s.tiles_y);
    if (tiles == 0 || tiles > 0x7fffffffLL) return DASR_E_UNSUPPORTED;
    if (((uintptr_t)workspace & 7) != 0) return DASR_E_SHAPE;
    if (workspace_bytes < dasr_image_metrics_u8_workspace(B, H, W, C, crop)) return DASR_E_WORKSPACE;
    s.a = a; s.b = b;
    s.part_ssd = (unsigned long long*)workspace;
    s.part = (double*)(s.part_ssd + (size_t)B * tiles);
    s.H = H; s.W = W; s.C = C; s.crop = crop; s.Hc = H - 2 * crop; s.Wc = W - 2 * crop;
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        s.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += s.g[i];
    }
    for (int i = 0; i < 11; ++i) s.g[i] /= sum;
    DASR_LAUNCH(k_image_metrics, dim3((unsigned)tiles, B), dim3(256), 0, stream, s);
    DASR_LAUNCH(k_image_metrics_final, dim3(B), dim3(256), 0, stream, (const unsigned long long*)s.part_ssd,
                (const double*)s.part, ssd, sums, (int)tiles);
    DASR_RETURN_LAUNCH_STATUS();
}
