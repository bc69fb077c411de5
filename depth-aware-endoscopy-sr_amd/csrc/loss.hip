// loss.hip — one-pass sums for the harness losses: the L1 pixel loss and the per-region
// smooth-L1 numerators / areas of dynamic_weight_mask_loss (codes/models/modules/mask_loss.py:64-90,
// F_model_depthCond.py:164,188-190).  The reference makes 10 masked passes over two [B,3,sH,sW] tensors; with
// one-hot depth masks every HR pixel belongs to at most one region (nearest upsampling of the mask:
// region[y/s][x/s]), so one pass yields all K numerators, the K areas and sum|sr-hr|; the division, the softmax
// weighting and the trainable weights stay in PyTorch (harness.py).  HBM-bound: 24 B per HR pixel forward,
// 36 B backward.  sr / hr are the API's NCHW tensors.
//
// Soft masks (any float values; the second half of this file): the mask sits INSIDE the smooth-L1,
// num_k = sum smooth_l1(M_k * (sr-hr)), so a pixel contributes to every region.  One thread takes one LR-pixel-wide run
// of s HR pixels in ALL C channels: it loads the run's K mask values once and keeps the K numerators (and the K areas,
// summed at LR: rows with Y % s == 0 only) in registers - the kernels are instantiated per K so that every per-k loop is
// unrolled.  8 B per HR element forward, 12 B backward, plus the LR planes; ~7 K VALU per element.
#include <stdint.h>

#include "dasr_common.h"

#define LOSS_MAXK 16

// sums: [0..K-1] numerators  sum smooth_l1(sr-hr) over the region (all channels)
//       [K..2K-1] areas       C * (#pixels of the region)          (= sum of the 3-channel mask, mask_loss.py:81)
//       [2K]      sum |sr - hr|
__global__ void __launch_bounds__(256) k_loss_sums(const float* __restrict__ sr, const float* __restrict__ hr,
                                                   const unsigned char* __restrict__ region, float* __restrict__ sums,
                                                   int B, int C, int h, int w, int s, int K) {
    __shared__ float red[2 * LOSS_MAXK + 2];
    for (int i = threadIdx.x; i < 2 * K + 1; i += 256) red[i] = 0.f;
    __syncthreads();
    const int W = w * s, H = h * s;
    // one thread = one LR-pixel-wide run of s HR pixels in one row of one channel: a single region
    const size_t nruns = (size_t)B * C * H * w;
    float l1 = 0.f;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        const int lx = (int)(r % w);
        const int Y = (int)((r / w) % H);
        const size_t bc = r / ((size_t)w * H);
        const int b = (int)(bc / C);
        const int k = region[((size_t)b * h + Y / s) * w + lx];
        const float* ps = sr + (bc * H + Y) * W + (size_t)lx * s;
        const float* ph = hr + (bc * H + Y) * W + (size_t)lx * s;
        float num = 0.f;
        for (int j = 0; j < s; ++j) {
            const float d = ps[j] - ph[j], ad = fabsf(d);
            l1 += ad;
            num += ad < 1.f ? 0.5f * d * d : ad - 0.5f;       // SmoothL1Loss(beta = 1)
        }
        if (k < K) {
            atomicAdd(&red[k], num);
            atomicAdd(&red[K + k], (float)s);
        }
    }
    for (int off = 32; off > 0; off >>= 1) l1 += __shfl_down(l1, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], l1);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * K + 1; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * sign(d) + dsums[region] * smooth_l1'(d)
__global__ void __launch_bounds__(256) k_loss_bwd(const float* __restrict__ sr, const float* __restrict__ hr,
                                                  const unsigned char* __restrict__ region,
                                                  const float* __restrict__ dsums, float* __restrict__ dsr, int B,
                                                  int C, int h, int w, int s, int K) {
    const int W = w * s, H = h * s;
    const size_t n = (size_t)B * C * H * W;
    const float dl1 = dsums[2 * K];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int X = (int)(i % W), Y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H * C));
        const int k = region[((size_t)b * h + Y / s) * w + X / s];
        const float d = sr[i] - hr[i];
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        float g = dl1 * sg;
        if (k < K) g += dsums[k] * (fabsf(d) < 1.f ? d : sg);
        dsr[i] = g;
    }
}

extern "C" int dasr_loss_sums(const float* sr, const float* hr, const unsigned char* region, float* sums, int B, int C,
                              int h, int w, int scale, int K, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(region); DASR_CHECK_PTR(sums);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    if (K > LOSS_MAXK) return DASR_E_UNSUPPORTED;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * (2 * K + 1), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    size_t nruns = (size_t)B * C * h * scale * w;
    DASR_LAUNCH(k_loss_sums, dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, sr, hr, region, sums, B, C, h, w, scale, K);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_loss_bwd(const float* sr, const float* hr, const unsigned char* region, const float* dsums,
                             float* dsr, int B, int C, int h, int w, int scale, int K, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(region); DASR_CHECK_PTR(dsums); DASR_CHECK_PTR(dsr);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    if (K > LOSS_MAXK) return DASR_E_UNSUPPORTED;
    size_t n = (size_t)B * C * h * scale * w * scale;
    DASR_LAUNCH(k_loss_bwd, dim3(dasr_ew_grid(n)), dim3(256), 0, stream, sr, hr, region, dsums, dsr, B, C, h, w, scale, K);
    DASR_RETURN_LAUNCH_STATUS();
}

// ---- soft masks ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float loss_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

template <int K>
__device__ __forceinline__ void loss_soft_px(float d, const float (&m)[K], float (&num)[K], float& l1) {
    l1 += fabsf(d);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d, au = fabsf(u);
        num[k] += au < 1.f ? 0.5f * u * u : au - 0.5f;        // SmoothL1Loss(beta = 1) of the MASKED difference
    }
}

template <int K>
__device__ __forceinline__ float loss_soft_px_bwd(float d, float dl1, const float (&m)[K], const float (&coef)[K]) {
    float g = dl1 * loss_sign(d);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d;
        g += coef[k] * (fabsf(u) < 1.f ? u : (u > 0.f ? 1.f : -1.f));
    }
    return g;
}

// run r of B*H*w -> (b, Y, lx); the K mask values of its LR pixel; offset of its first HR pixel in channel 0
template <int K>
__device__ __forceinline__ size_t loss_soft_run(size_t r, const float* __restrict__ mask, int C, int h, int w, int s,
                                                float (&m)[K], bool& first_row) {
    const int H = h * s;
    const int lx = (int)(r % w);
    const int Y = (int)((r / w) % H);
    const size_t b = r / ((size_t)w * H);
    const int y = Y / s;
    first_row = Y == y * s;
    const float* pm = mask + ((b * K) * h + y) * w + lx;
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = pm[(size_t)k * h * w];
    return ((b * C) * H + Y) * ((size_t)w * s) + (size_t)lx * s;
}

// VEC: s % 4 == 0 and 16-byte aligned tensors, so every run starts on a 16-byte boundary (W = w * s)
template <int K, bool VEC>
__global__ void __launch_bounds__(256) k_loss_sums_soft(const float* __restrict__ sr, const float* __restrict__ hr,
                                                        const float* __restrict__ mask, float* __restrict__ sums, int B,
                                                        int C, int h, int w, int s) {
    __shared__ float red[2 * LOSS_MAXK + 1];
    for (int i = threadIdx.x; i < 2 * K + 1; i += 256) red[i] = 0.f;
    __syncthreads();
    const size_t plane = (size_t)h * s * w * s;
    const size_t nruns = (size_t)B * h * s * w;
    float num[K], area[K], m[K], l1 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) num[k] = area[k] = 0.f;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        bool first_row;
        const size_t off = loss_soft_run<K>(r, mask, C, h, w, s, m, first_row);
        if (first_row) {                                       // the areas are sums at LR: once per LR pixel
#pragma unroll
            for (int k = 0; k < K; ++k) area[k] += m[k];
        }
        for (int c = 0; c < C; ++c) {
            const float* ps = sr + off + c * plane;
            const float* ph = hr + off + c * plane;
            if (VEC) {
                for (int j = 0; j < s; j += 4) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(ps + j) - *reinterpret_cast<const f32x4*>(ph + j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) loss_soft_px<K>(d[i], m, num, l1);
                }
            } else {
                for (int j = 0; j < s; ++j) loss_soft_px<K>(ps[j] - ph[j], m, num, l1);
            }
        }
    }
    // wave reduction, then ONE LDS atomic per wave and sum, then one global atomic per workgroup and sum
    const float area_scale = (float)C * (float)s * (float)s;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float a = num[k], b = area[k];
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&red[k], a);
            atomicAdd(&red[K + k], b * area_scale);
        }
    }
    for (int off = 32; off > 0; off >>= 1) l1 += __shfl_down(l1, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], l1);
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * K + 1; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * sign(d) + sum_k dsums[k] * M_k * smooth_l1'(M_k * d)
template <int K, bool VEC>
__global__ void __launch_bounds__(256) k_loss_bwd_soft(const float* __restrict__ sr, const float* __restrict__ hr,
                                                       const float* __restrict__ mask, const float* __restrict__ dsums,
                                                       float* __restrict__ dsr, int B, int C, int h, int w, int s) {
    const size_t plane = (size_t)h * s * w * s;
    const size_t nruns = (size_t)B * h * s * w;
    float dnum[K], m[K], coef[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dnum[k] = dsums[k];
    const float dl1 = dsums[2 * K];
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        bool first_row;
        const size_t off = loss_soft_run<K>(r, mask, C, h, w, s, m, first_row);
#pragma unroll
        for (int k = 0; k < K; ++k) coef[k] = dnum[k] * m[k];
        for (int c = 0; c < C; ++c) {
            const float* ps = sr + off + c * plane;
            const float* ph = hr + off + c * plane;
            float* pd = dsr + off + c * plane;
            if (VEC) {
                for (int j = 0; j < s; j += 4) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(ps + j) - *reinterpret_cast<const f32x4*>(ph + j);
                    f32x4 g;
#pragma unroll
                    for (int i = 0; i < 4; ++i) g[i] = loss_soft_px_bwd<K>(d[i], dl1, m, coef);
                    *reinterpret_cast<f32x4*>(pd + j) = g;
                }
            } else {
                for (int j = 0; j < s; ++j) pd[j] = loss_soft_px_bwd<K>(ps[j] - ph[j], dl1, m, coef);
            }
        }
    }
}

static inline bool loss_aligned16(const void* a, const void* b, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// one instantiation per K (1 .. LOSS_MAXK) and load width
#define LOSS_SOFT_CASE(KK, KERNEL, ...)                                                                  \
    case KK:                                                                                             \
        if (vec) DASR_LAUNCH((KERNEL<KK, true>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);  \
        else DASR_LAUNCH((KERNEL<KK, false>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);     \
        break;
#define LOSS_SOFT_DISPATCH(KERNEL, ...)                                                                          \
    switch (K) {                                                                                                 \
        LOSS_SOFT_CASE(1, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(2, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(3, KERNEL, __VA_ARGS__)    \
        LOSS_SOFT_CASE(4, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(5, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(6, KERNEL, __VA_ARGS__)    \
        LOSS_SOFT_CASE(7, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(8, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(9, KERNEL, __VA_ARGS__)    \
        LOSS_SOFT_CASE(10, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(11, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(12, KERNEL, __VA_ARGS__) \
        LOSS_SOFT_CASE(13, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(14, KERNEL, __VA_ARGS__) LOSS_SOFT_CASE(15, KERNEL, __VA_ARGS__) \
        LOSS_SOFT_CASE(16, KERNEL, __VA_ARGS__)                                                                  \
        default: return DASR_E_UNSUPPORTED;                                                                      \
    }

extern "C" int dasr_loss_sums_soft(const float* sr, const float* hr, const float* mask, float* sums, int B, int C, int h,
                                   int w, int scale, int K, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(mask); DASR_CHECK_PTR(sums);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    if (K > LOSS_MAXK) return DASR_E_UNSUPPORTED;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * (2 * K + 1), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const size_t nruns = (size_t)B * h * scale * w;
    const bool vec = scale % 4 == 0 && loss_aligned16(sr, hr);
    LOSS_SOFT_DISPATCH(k_loss_sums_soft, sr, hr, mask, sums, B, C, h, w, scale)
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_loss_bwd_soft(const float* sr, const float* hr, const float* mask, const float* dsums, float* dsr,
                                  int B, int C, int h, int w, int scale, int K, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(mask); DASR_CHECK_PTR(dsums); DASR_CHECK_PTR(dsr);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    if (K > LOSS_MAXK) return DASR_E_UNSUPPORTED;
    const size_t nruns = (size_t)B * h * scale * w;
    const bool vec = scale % 4 == 0 && loss_aligned16(sr, hr, dsr);
    LOSS_SOFT_DISPATCH(k_loss_bwd_soft, sr, hr, mask, dsums, dsr, B, C, h, w, scale)
    DASR_RETURN_LAUNCH_STATUS();
}

// ---- criterion-parametrised family (F_model_depthCond.py:50-58,164,183-190; mask_loss.py:6-41,44-90; loss.py:37-47) ----------
// The kernels above stay what the default configuration runs.  Here the pixel criterion (l1 | l2 | cb) and one or two region
// criteria (l1 | l2 | smoothl1: A for dynamic_weight_mask_loss, B for mask_loss when its criterion differs) are ARGUMENTS.
// A region criterion is not a branch: all three are  f(u) = |u| < thr ? a2 * u^2 : a1 * |u| + a0  with wave-uniform
// (thr, a2, a1, a0) = l1 (0, 0, 1, 0) | l2 (inf, 1, 0, 0) | smoothl1 (1, 1/2, 1, -1/2), the arithmetic of the smooth-L1 the
// kernels above hard-wire (bit for bit for smoothl1: 0.5f * u * u and |u| - 0.5f), so a criterion costs what smooth-L1 costs.
// f'(u) = |u| < thr ? 2 a2 u : a1 sign(u), sign(0) = 0.  The pixel criterion is evaluated once per element, not once per
// region: a wave-uniform branch (cb pays a sqrt).  Per-K / load-width instantiation as above, times {A, A and B}.
// sums: [0..K-1] A numerators | [K..2K-1] areas | [2K] pixel sum | with B: [2K+1..3K] B numerators.
struct LossCrit {
    float thr, a2, a1, a0;
};

static inline bool loss_region_crit(int code, LossCrit& c) {
    if (code == DASR_CRIT_L1) c = LossCrit{0.f, 0.f, 1.f, 0.f};
    else if (code == DASR_CRIT_L2) c = LossCrit{__builtin_inff(), 1.f, 0.f, 0.f};
    else if (code == DASR_CRIT_SMOOTHL1) c = LossCrit{1.f, 0.5f, 1.f, -0.5f};
    else return false;
    return true;
}
static inline bool loss_pixel_crit(int code) { return code == DASR_CRIT_L1 || code == DASR_CRIT_L2 || code == DASR_CRIT_CB; }

#define LOSS_CB_EPS 1e-6f                                        // CharbonnierLoss(eps) (loss.py:40)

__device__ __forceinline__ float loss_pix(float d, int pix) {
    if (pix == DASR_CRIT_CB) return sqrtf(d * d + LOSS_CB_EPS);
    if (pix == DASR_CRIT_L2) return d * d;
    return fabsf(d);
}
__device__ __forceinline__ float loss_pix_grad(float d, int pix) {
    if (pix == DASR_CRIT_CB) return d / sqrtf(d * d + LOSS_CB_EPS);
    if (pix == DASR_CRIT_L2) return 2.f * d;
    return loss_sign(d);
}
__device__ __forceinline__ float loss_crit(float u, const LossCrit& c) {
    const float au = fabsf(u);
    return au < c.thr ? c.a2 * u * u : c.a1 * au + c.a0;
}
__device__ __forceinline__ float loss_crit_grad(float u, const LossCrit& c) {
    return fabsf(u) < c.thr ? (2.f * c.a2) * u : c.a1 * loss_sign(u);
}

// one-hot region bytes: the thread layout of k_loss_sums
template <bool HAS_B>
__global__ void __launch_bounds__(256) k_loss_sums_crit(const float* __restrict__ sr, const float* __restrict__ hr,
                                                        const unsigned char* __restrict__ region,
                                                        float* __restrict__ sums, int B, int C, int h, int w, int s, int K,
                                                        int pix, LossCrit qa, LossCrit qb) {
    __shared__ float red[3 * LOSS_MAXK + 2];
    const int nsums = (HAS_B ? 3 : 2) * K + 1;
    for (int i = threadIdx.x; i < nsums; i += 256) red[i] = 0.f;
    __syncthreads();
    const int W = w * s, H = h * s;
    const size_t nruns = (size_t)B * C * H * w;
    float px = 0.f;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        const int lx = (int)(r % w);
        const int Y = (int)((r / w) % H);
        const size_t bc = r / ((size_t)w * H);
        const int b = (int)(bc / C);
        const int k = region[((size_t)b * h + Y / s) * w + lx];
        const float* ps = sr + (bc * H + Y) * W + (size_t)lx * s;
        const float* ph = hr + (bc * H + Y) * W + (size_t)lx * s;
        float na = 0.f, nb = 0.f;
        for (int j = 0; j < s; ++j) {
            const float d = ps[j] - ph[j];
            px += loss_pix(d, pix);
            na += loss_crit(d, qa);
            if (HAS_B) nb += loss_crit(d, qb);
        }
        if (k < K) {
            atomicAdd(&red[k], na);
            atomicAdd(&red[K + k], (float)s);
            if (HAS_B) atomicAdd(&red[2 * K + 1 + k], nb);
        }
    }
    for (int off = 32; off > 0; off >>= 1) px += __shfl_down(px, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], px);
    __syncthreads();
    for (int i = threadIdx.x; i < nsums; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * pix'(d) + dsums[region] * A'(d) (+ dsums[2K+1+region] * B'(d))
template <bool HAS_B>
__global__ void __launch_bounds__(256) k_loss_bwd_crit(const float* __restrict__ sr, const float* __restrict__ hr,
                                                       const unsigned char* __restrict__ region,
                                                       const float* __restrict__ dsums, float* __restrict__ dsr, int B,
                                                       int C, int h, int w, int s, int K, int pix, LossCrit qa,
                                                       LossCrit qb) {
    const int W = w * s, H = h * s;
    const size_t n = (size_t)B * C * H * W;
    const float dpx = dsums[2 * K];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int X = (int)(i % W), Y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H * C));
        const int k = region[((size_t)b * h + Y / s) * w + X / s];
        const float d = sr[i] - hr[i];
        float g = dpx * loss_pix_grad(d, pix);
        if (k < K) {
            g += dsums[k] * loss_crit_grad(d, qa);
            if (HAS_B) g += dsums[2 * K + 1 + k] * loss_crit_grad(d, qb);
        }
        dsr[i] = g;
    }
}

// soft masks: the thread layout of k_loss_sums_soft
template <int K, bool HAS_B>
__device__ __forceinline__ void loss_crit_px(float d, const float (&m)[K], float (&na)[K], float (&nb)[HAS_B ? K : 1],
                                             float& px, int pix, const LossCrit& qa, const LossCrit& qb) {
    px += loss_pix(d, pix);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d;
        na[k] += loss_crit(u, qa);
        if (HAS_B) nb[k] += loss_crit(u, qb);
    }
}

template <int K, bool HAS_B>
__device__ __forceinline__ float loss_crit_px_bwd(float d, float dpx, const float (&m)[K], const float (&fa)[K],
                                                  const float (&fb)[HAS_B ? K : 1], int pix, const LossCrit& qa,
                                                  const LossCrit& qb) {
    float g = dpx * loss_pix_grad(d, pix);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d;
        g += fa[k] * loss_crit_grad(u, qa);
        if (HAS_B) g += fb[k] * loss_crit_grad(u, qb);
    }
    return g;
}

template <int K, bool VEC, bool HAS_B>
__global__ void __launch_bounds__(256) k_loss_sums_soft_crit(const float* __restrict__ sr, const float* __restrict__ hr,
                                                             const float* __restrict__ mask, float* __restrict__ sums,
                                                             int B, int C, int h, int w, int s, int pix, LossCrit qa,
                                                             LossCrit qb) {
    constexpr int KB = HAS_B ? K : 1;
    constexpr int NSUMS = (HAS_B ? 3 : 2) * K + 1;
    __shared__ float red[3 * LOSS_MAXK + 1];
    for (int i = threadIdx.x; i < NSUMS; i += 256) red[i] = 0.f;
    __syncthreads();
    const size_t plane = (size_t)h * s * w * s;
    const size_t nruns = (size_t)B * h * s * w;
    float na[K], nb[KB], area[K], m[K], px = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) na[k] = area[k] = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) nb[k] = 0.f;
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        bool first_row;
        const size_t off = loss_soft_run<K>(r, mask, C, h, w, s, m, first_row);
        if (first_row) {
#pragma unroll
            for (int k = 0; k < K; ++k) area[k] += m[k];
        }
        for (int c = 0; c < C; ++c) {
            const float* ps = sr + off + c * plane;
            const float* ph = hr + off + c * plane;
            if (VEC) {
                for (int j = 0; j < s; j += 4) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(ps + j) - *reinterpret_cast<const f32x4*>(ph + j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) loss_crit_px<K, HAS_B>(d[i], m, na, nb, px, pix, qa, qb);
                }
            } else {
                for (int j = 0; j < s; ++j) loss_crit_px<K, HAS_B>(ps[j] - ph[j], m, na, nb, px, pix, qa, qb);
            }
        }
    }
    const float area_scale = (float)C * (float)s * (float)s;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float a = na[k], b = area[k], c = HAS_B ? nb[HAS_B ? k : 0] : 0.f;
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
            if (HAS_B) c += __shfl_down(c, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&red[k], a);
            atomicAdd(&red[K + k], b * area_scale);
            if (HAS_B) atomicAdd(&red[2 * K + 1 + k], c);
        }
    }
    for (int off = 32; off > 0; off >>= 1) px += __shfl_down(px, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], px);
    __syncthreads();
    for (int i = threadIdx.x; i < NSUMS; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * pix'(d) + sum_k M_k * (dsums[k] * A'(M_k d) + dsums[2K+1+k] * B'(M_k d))
template <int K, bool VEC, bool HAS_B>
__global__ void __launch_bounds__(256) k_loss_bwd_soft_crit(const float* __restrict__ sr, const float* __restrict__ hr,
                                                            const float* __restrict__ mask,
                                                            const float* __restrict__ dsums, float* __restrict__ dsr,
                                                            int B, int C, int h, int w, int s, int pix, LossCrit qa,
                                                            LossCrit qb) {
    constexpr int KB = HAS_B ? K : 1;
    const size_t plane = (size_t)h * s * w * s;
    const size_t nruns = (size_t)B * h * s * w;
    float da[K], db[KB], m[K], fa[K], fb[KB];
#pragma unroll
    for (int k = 0; k < K; ++k) da[k] = dsums[k];
#pragma unroll
    for (int k = 0; k < KB; ++k) db[k] = HAS_B ? dsums[2 * K + 1 + k] : 0.f;
    const float dpx = dsums[2 * K];
    for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < nruns; r += (size_t)gridDim.x * 256) {
        bool first_row;
        const size_t off = loss_soft_run<K>(r, mask, C, h, w, s, m, first_row);
#pragma unroll
        for (int k = 0; k < K; ++k) fa[k] = da[k] * m[k];
#pragma unroll
        for (int k = 0; k < KB; ++k) fb[k] = db[k] * m[k];
        for (int c = 0; c < C; ++c) {
            const float* ps = sr + off + c * plane;
            const float* ph = hr + off + c * plane;
            float* pd = dsr + off + c * plane;
            if (VEC) {
                for (int j = 0; j < s; j += 4) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(ps + j) - *reinterpret_cast<const f32x4*>(ph + j);
                    f32x4 g;
#pragma unroll
                    for (int i = 0; i < 4; ++i) g[i] = loss_crit_px_bwd<K, HAS_B>(d[i], dpx, m, fa, fb, pix, qa, qb);
                    *reinterpret_cast<f32x4*>(pd + j) = g;
                }
            } else {
                for (int j = 0; j < s; ++j) pd[j] = loss_crit_px_bwd<K, HAS_B>(ps[j] - ph[j], dpx, m, fa, fb, pix, qa, qb);
            }
        }
    }
}

// codes -> coefficients; anything the family does not compute is refused before a launch
#define LOSS_CRIT_SETUP()                                                                                        \
    LossCrit qa, qb = LossCrit{0.f, 0.f, 0.f, 0.f};                                                              \
    if (K > LOSS_MAXK || !loss_pixel_crit(pixel_crit) || !loss_region_crit(crit_a, qa)) return DASR_E_UNSUPPORTED; \
    const bool has_b = crit_b != DASR_CRIT_NONE;                                                                 \
    if (has_b && !loss_region_crit(crit_b, qb)) return DASR_E_UNSUPPORTED;

#define LOSS_CRIT_CASE(KK, KERNEL, ...)                                                                           \
    case KK:                                                                                                      \
        if (vec && has_b) DASR_LAUNCH((KERNEL<KK, true, true>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);        \
        else if (vec) DASR_LAUNCH((KERNEL<KK, true, false>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);         \
        else if (has_b) DASR_LAUNCH((KERNEL<KK, false, true>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);       \
        else DASR_LAUNCH((KERNEL<KK, false, false>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);                 \
        break;
#define LOSS_CRIT_DISPATCH(KERNEL, ...)                                                                          \
    switch (K) {                                                                                                 \
        LOSS_CRIT_CASE(1, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(2, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(3, KERNEL, __VA_ARGS__)    \
        LOSS_CRIT_CASE(4, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(5, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(6, KERNEL, __VA_ARGS__)    \
        LOSS_CRIT_CASE(7, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(8, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(9, KERNEL, __VA_ARGS__)    \
        LOSS_CRIT_CASE(10, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(11, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(12, KERNEL, __VA_ARGS__) \
        LOSS_CRIT_CASE(13, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(14, KERNEL, __VA_ARGS__) LOSS_CRIT_CASE(15, KERNEL, __VA_ARGS__) \
        LOSS_CRIT_CASE(16, KERNEL, __VA_ARGS__)                                                                  \
        default: return DASR_E_UNSUPPORTED;                                                                      \
    }

extern "C" int dasr_loss_sums_crit(const float* sr, const float* hr, const unsigned char* region, float* sums, int B,
                                   int C, int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b,
                                   void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(region); DASR_CHECK_PTR(sums);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    LOSS_CRIT_SETUP()
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * ((has_b ? 3 : 2) * K + 1), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    size_t nruns = (size_t)B * C * h * scale * w;
    if (has_b) DASR_LAUNCH((k_loss_sums_crit<true>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, sr, hr, region, sums, B, C, h, w, scale, K, pixel_crit, qa, qb);
    else DASR_LAUNCH((k_loss_sums_crit<false>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, sr, hr, region, sums, B, C, h, w, scale, K, pixel_crit, qa, qb);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_loss_bwd_crit(const float* sr, const float* hr, const unsigned char* region, const float* dsums,
                                  float* dsr, int B, int C, int h, int w, int scale, int K, int pixel_crit, int crit_a,
                                  int crit_b, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(region); DASR_CHECK_PTR(dsums); DASR_CHECK_PTR(dsr);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    LOSS_CRIT_SETUP()
    size_t n = (size_t)B * C * h * scale * w * scale;
    if (has_b) DASR_LAUNCH((k_loss_bwd_crit<true>), dim3(dasr_ew_grid(n)), dim3(256), 0, stream, sr, hr, region, dsums, dsr, B, C, h, w, scale, K, pixel_crit, qa, qb);
    else DASR_LAUNCH((k_loss_bwd_crit<false>), dim3(dasr_ew_grid(n)), dim3(256), 0, stream, sr, hr, region, dsums, dsr, B, C, h, w, scale, K, pixel_crit, qa, qb);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_loss_sums_soft_crit(const float* sr, const float* hr, const float* mask, float* sums, int B, int C,
                                        int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b,
                                        void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(mask); DASR_CHECK_PTR(sums);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    LOSS_CRIT_SETUP()
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * ((has_b ? 3 : 2) * K + 1), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    const size_t nruns = (size_t)B * h * scale * w;
    const bool vec = scale % 4 == 0 && loss_aligned16(sr, hr);
    LOSS_CRIT_DISPATCH(k_loss_sums_soft_crit, sr, hr, mask, sums, B, C, h, w, scale, pixel_crit, qa, qb)
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_loss_bwd_soft_crit(const float* sr, const float* hr, const float* mask, const float* dsums,
                                       float* dsr, int B, int C, int h, int w, int scale, int K, int pixel_crit,
                                       int crit_a, int crit_b, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(mask); DASR_CHECK_PTR(dsums); DASR_CHECK_PTR(dsr);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && scale > 0 && K > 0);
    LOSS_CRIT_SETUP()
    const size_t nruns = (size_t)B * h * scale * w;
    const bool vec = scale % 4 == 0 && loss_aligned16(sr, hr, dsr);
    LOSS_CRIT_DISPATCH(k_loss_bwd_soft_crit, sr, hr, mask, dsums, dsr, B, C, h, w, scale, pixel_crit, qa, qb)
    DASR_RETURN_LAUNCH_STATUS();
}
