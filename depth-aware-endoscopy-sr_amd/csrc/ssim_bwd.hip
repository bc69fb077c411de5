// ssim_bwd.hip — gradient of the SSIM criterion (reference models/modules/ssim_loss.py, used at F_model_depthCond.py:179)
// with respect to its first image, in ONE launch that saves nothing between forward and backward.
//
// S = mean_p s_p with s = A1 A2 / (B1 B2), A1 = 2 mu1 mu2 + C1, A2 = 2 (m12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1,
// B2 = (m11 - mu1^2) + (m22 - mu2^2) + C2 and the five moments mu1 = G*x, mu2 = G*y, m11 = G*x^2, m22 = G*y^2, m12 = G*xy
// (G: the zero-padded separable 11 x 11 window of ssim.hip).  G is symmetric and its zero padding self-adjoint, so
//     dS/dx_q = 1/N [ (G*a)_q + 2 x_q (G*b)_q + y_q (G*c)_q ]
//     a = ds/dmu1 = 2 mu2 (A2 - A1) / (B1 B2) - 2 mu1 s / B1 + 2 mu1 s / B2,   b = ds/dm11 = -s / B2,   c = ds/dm12 = 2 A1 / (B1 B2)
// with a, b, c zero outside the image.  A workgroup owns a 32 x 32 tile of one plane:
//   1. stage the radius-10 halo (52 x 52) of x and y in LDS, zeros outside the image;
//   2. filter the five products horizontally: 52 rows x 42 columns;
//   3. filter them vertically onto the radius-5 halo (42 x 42) and form a, b, c there - into the LDS the images occupied,
//      which are dead by then (each thread has taken its own x_q, y_q into registers);
//   4. filter a, b, c horizontally (42 rows x 32 columns) into the LDS of step 2, then vertically onto the tile, and write.
// In the vertical passes a thread owns a strip of one column (7 rows in step 3, 4 rows in step 4) and reads the 17 / 14 words
// it needs once into registers: 2.4 / 3.5 LDS reads per output and moment instead of 11.
// The radius-5 ring is recomputed by the neighbouring tiles (LDS reads and VALU) instead of a, b, c going through HBM.
// LDS: 2 * 52 * 52 + 5 * 52 * 42 floats = 65 312 bytes, two workgroups per CU.  Rows are stored dense: every write and
// every vertical read then has consecutive lanes on consecutive words (no two lanes of a 32-lane group on one bank); the
// horizontal reads skip 10 words where a wave crosses a row end, at most 10 lanes of a group two-way.
// Each output element is written by exactly one thread: no atomics, bit-identical from run to run.
#include "dasr_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

#define SB_T 32
#define SB_R 5
#define SB_H1 (SB_T + 2 * SB_R)        // 42: the tile with the radius-5 halo (where a, b, c are needed)
#define SB_H2 (SB_T + 4 * SB_R)        // 52: with the radius-10 halo (what the moments there read)
#define SB_IMG_FLOATS (2 * SB_H2 * SB_H2)          // x | y; later a | b | c (3 * 42 * 42 <= 2 * 52 * 52)
#define SB_HZ_FLOATS (5 * SB_H2 * SB_H1)           // five moments after the horizontal pass; later a, b, c after theirs

struct SsimBwdArgs {
    const float* x;
    const float* y;
    const float* dscale;   // device, one float: dL/dS
    float* dx;
    int H, W, tiles_x, accumulate;
    float count;           // B C H W
    float g[11];
};

__global__ void __launch_bounds__(256) k_ssim_bwd_tiles(SsimBwdArgs s) {
    __shared__ float sImg[SB_IMG_FLOATS];
    __shared__ float sHz[SB_HZ_FLOATS];
    static_assert(3 * SB_H1 * SB_H1 <= SB_IMG_FLOATS && 3 * SB_H1 * SB_T <= SB_HZ_FLOATS, "aliased buffers must fit");
    float* const sX = sImg;
    float* const sY = sImg + SB_H2 * SB_H2;
    const int tid = threadIdx.x, plane = blockIdx.y;
    const int tile = blockIdx.x, tx = tile % s.tiles_x, ty = tile / s.tiles_x;
    const int x0 = tx * SB_T, y0 = ty * SB_T;
    const size_t base = (size_t)plane * s.H * s.W;
    const float* px = s.x + base;
    const float* py = s.y + base;
    // 1. the radius-10 halo of both images
    for (int i = tid; i < SB_H2 * SB_H2; i += 256) {
        const int r = i / SB_H2, c = i - r * SB_H2;
        const int gy = y0 + r - 2 * SB_R, gx = x0 + c - 2 * SB_R;
        const bool in = gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
        sX[i] = in ? px[(size_t)gy * s.W + gx] : 0.f;
        sY[i] = in ? py[(size_t)gy * s.W + gx] : 0.f;
    }
    __syncthreads();
    // this thread's four output pixels (column tc, rows tr0 .. tr0 + 3 of the tile): their x and y leave LDS before a, b, c
    // overwrite the images
    const int tc = tid & (SB_T - 1), tr0 = (tid >> 5) * 4;
    float xq[4], yq[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        xq[u] = sX[(tr0 + u + 2 * SB_R) * SB_H2 + tc + 2 * SB_R];
        yq[u] = sY[(tr0 + u + 2 * SB_R) * SB_H2 + tc + 2 * SB_R];
    }
    // 2. horizontal pass of the five products: sHz[q][r][c], r a row of the 52-halo, c a column of the 42-halo
    for (int i = tid; i < SB_H2 * SB_H1; i += 256) {
        const int r = i / SB_H1, c = i - r * SB_H1;
        // (x, y) and (x^2, y^2) as two-element vectors: gfx950 has packed fp32 multiply and fma at the scalar forms' rate
        f32x2 mu = {0.f, 0.f}, sq = {0.f, 0.f};
        float q12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const f32x2 v = {sX[r * SB_H2 + c + k], sY[r * SB_H2 + c + k]};
            const float w = s.g[k];
            mu += w * v;
            sq += w * (v * v);
            q12 += w * (v.x * v.y);
        }
        const float m1 = mu.x, m2 = mu.y, q11 = sq.x, q22 = sq.y;
        sHz[i] = m1;
        sHz[SB_H2 * SB_H1 + i] = m2;
        sHz[2 * SB_H2 * SB_H1 + i] = q11;
        sHz[3 * SB_H2 * SB_H1 + i] = q22;
        sHz[4 * SB_H2 * SB_H1 + i] = q12;
    }
    __syncthreads();
    // 3. vertical pass onto the 42-halo; a, b, c there (zero outside the image), into the images' LDS
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float* const sA = sImg;
    float* const sB = sImg + SB_H1 * SB_H1;
    float* const sC = sImg + 2 * SB_H1 * SB_H1;
    // a thread takes 7 consecutive rows of one column (6 strips x 42 columns = 252 threads): the 17 words of the column it
    // needs per moment are read once into registers instead of 11 per output
    if (tid < 6 * SB_H1) {
        const int strip = tid / SB_H1, c = tid - strip * SB_H1, r0 = 7 * strip;
        const int gx = x0 + c - SB_R;
        float m[5][7];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float v[17];
#pragma unroll
            for (int j = 0; j < 17; ++j) v[j] = sHz[q * SB_H2 * SB_H1 + (r0 + j) * SB_H1 + c];
#pragma unroll
            for (int o = 0; o < 7; ++o) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc += s.g[k] * v[o + k];
                m[q][o] = acc;
            }
        }
#pragma unroll
        for (int o = 0; o < 7; ++o) {
            const int gy = y0 + r0 + o - SB_R;
            const bool in = gy >= 0 && gy < s.H && gx >= 0 && gx < s.W;
            const float mu1 = m[0][o], mu2 = m[1][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float A1 = 2.f * mu12 + C1, A2 = 2.f * (m[4][o] - mu12) + C2;
            const float B1 = mu1_sq + mu2_sq + C1, B2 = (m[2][o] - mu1_sq) + (m[3][o] - mu2_sq) + C2;
            const float rB1 = 1.f / B1, rB2 = 1.f / B2, rB = rB1 * rB2;
            const float sv = A1 * A2 * rB;
            const float a = 2.f * mu2 * (A2 - A1) * rB + 2.f * mu1 * sv * (rB2 - rB1);
            const int i = (r0 + o) * SB_H1 + c;
            sA[i] = in ? a : 0.f;
            sB[i] = in ? -sv * rB2 : 0.f;
            sC[i] = in ? 2.f * A1 * rB : 0.f;
        }
    }
    __syncthreads();
    // 4a. horizontal pass of a, b, c: 42 rows x 32 columns, into the moments' LDS
    float* const hA = sHz;
    float* const hB = sHz + SB_H1 * SB_T;
    float* const hC = sHz + 2 * SB_H1 * SB_T;
    for (int i = tid; i < SB_H1 * SB_T; i += 256) {
        const int r = i / SB_T, c = i - r * SB_T;
        float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float w = s.g[k];
            fa += w * sA[r * SB_H1 + c + k];
            fb += w * sB[r * SB_H1 + c + k];
            fc += w * sC[r * SB_H1 + c + k];
        }
        hA[i] = fa; hB[i] = fb; hC[i] = fc;
    }
    __syncthreads();
    // 4b. vertical pass onto the tile and the product rule
    const float scale = s.dscale[0] / s.count;
    float* pd = s.dx + base;
    float f[3][4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float v[14];
#pragma unroll
        for (int j = 0; j < 14; ++j) v[j] = sHz[q * SB_H1 * SB_T + (tr0 + j) * SB_T + tc];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) acc += s.g[k] * v[u + k];
            f[q][u] = acc;
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int gy = y0 + tr0 + u, gx = x0 + tc;
        if (gy >= s.H || gx >= s.W) continue;
        const float t = f[0][u] + 2.f * xq[u] * f[1][u] + yq[u] * f[2][u];
        // A statement of its own: the library is built with -ffp-contract=on (build.py), which fuses within an expression only,
        // so scale * t is rounded before the add below and the accumulating form adds the SAME value the plain form writes.
        // (Under hipcc's default -ffp-contract=fast the two statements could become one fma and differ in the last bit.)
        float v = scale * t;
        const size_t o = (size_t)gy * s.W + gx;
        if (s.accumulate) v = pd[o] + v;
        pd[o] = v;
    }
}

extern "C" int dasr_ssim_bwd(const float* img1, const float* img2, const float* window11, const float* dscale, float* dimg1,
                             int accumulate, int B, int C, int H, int W, void* stream) {
    DASR_CHECK_PTR(img1); DASR_CHECK_PTR(img2); DASR_CHECK_PTR(window11); DASR_CHECK_PTR(dscale); DASR_CHECK_PTR(dimg1);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && H > 0 && W > 0 && (size_t)B * C <= 65535);
    SsimBwdArgs s;
    s.x = img1; s.y = img2; s.dscale = dscale; s.dx = dimg1;
    s.H = H; s.W = W; s.accumulate = accumulate ? 1 : 0;
    s.tiles_x = (W + SB_T - 1) / SB_T;
    const size_t tiles = (size_t)s.tiles_x * ((H + SB_T - 1) / SB_T);
    DASR_CHECK_SHAPE(tiles <= 0x7fffffffu);
    s.count = (float)((double)B * C * H * W);
    for (int i = 0; i < 11; ++i) s.g[i] = window11[i];          // (host pointer: eleven floats, passed by value)
    DASR_LAUNCH(k_ssim_bwd_tiles, dim3((unsigned)tiles, B * C), dim3(256), 0, stream, s);
    DASR_RETURN_LAUNCH_STATUS();
}
