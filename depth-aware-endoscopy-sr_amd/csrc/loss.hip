// loss.hip — one-pass sums for the harness losses: the pixel loss and the per-region numerators /
// areas of dynamic_weight_mask_loss and mask_loss (codes/models/modules/mask_loss.py:6-41,44-90, loss.py:37-47,
// F_model_depthCond.py:50-58,164,183-190).  The reference makes 10 masked passes over two [B,3,sH,sW] tensors; here one
// pass yields every numerator, the K areas and the pixel sum; the division, the softmax weighting and the trainable
// weights stay in PyTorch (harness.py).  sr / hr are the API's NCHW tensors.
//
// ONE family of four loops, each written once:
//   * one-hot masks (region bytes from dasr_mask_compress): every HR pixel belongs to at most one region (nearest upsampling
//     of the mask: region[y/s][x/s]).  HBM-bound: 24 B per HR pixel forward, 36 B backward.
//   * soft masks (any float values): the mask sits INSIDE the criterion, num_k = sum f(M_k * (sr-hr)), so a pixel contributes
//     to every region.  One thread takes one LR-pixel-wide run of s HR pixels in ALL C channels: it loads the run's K mask
//     values once and keeps the K numerators (and the K areas, summed at LR: rows with Y % s == 0 only) in registers - the
//     kernels are instantiated per K so that every per-k loop is unrolled.  8 B per HR element forward, 12 B backward, plus
//     the LR planes; ~7 K VALU per element.
// and TWO criterion policies the loops are templated on:
//   * LossFixed: pixel l1, region smooth-L1, no second numerator set, all at compile time - what the default configuration
//     runs (dasr_loss_{sums,bwd}[_soft]).
//   * LossArgs<HAS_B>: the pixel criterion (l1 | l2 | cb) and one or two region criteria (l1 | l2 | smoothl1: A for
//     dynamic_weight_mask_loss, B for mask_loss when its criterion differs) are kernel ARGUMENTS
//     (dasr_loss_{sums,bwd}[_soft]_crit, the default codes included).  A region criterion is not a branch: all three are
//     f(u) = |u| < thr ? a2 * u^2 : a1 * |u| + a0  with wave-uniform (thr, a2, a1, a0) = l1 (0, 0, 1, 0) | l2 (inf, 1, 0, 0) |
//     smoothl1 (1, 1/2, 1, -1/2), the arithmetic of LossFixed's smooth-L1 (bit for bit for smoothl1: 0.5f * u * u and
//     |u| - 0.5f), so a criterion costs what smooth-L1 costs.  f'(u) = |u| < thr ? 2 a2 u : a1 sign(u), sign(0) = 0.  The
//     pixel criterion is evaluated once per element, not once per region: a wave-uniform branch (cb pays a sqrt).
// sums: [0..K-1]    A numerators  sum f_A(M_k (sr-hr)) over all channels
//       [K..2K-1]   areas         C * sum M_k at HR              (= sum of the 3-channel mask, mask_loss.py:81)
//       [2K]        the pixel criterion's sum
//       [2K+1..3K]  B numerators  (LossArgs<true> only)
#include <stdint.h>

#include <type_traits>

#include "dasr_common.h"

#define LOSS_MAXK 16
#define LOSS_CB_EPS 1e-6f                                        // CharbonnierLoss(eps) (loss.py:40)

__device__ __forceinline__ float loss_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// ---- criterion policies ------------------------------------------------------------------------------------------------
struct LossFixed {
    static constexpr bool HAS_B = false;
    static constexpr int LDS_SETS = 2;                           // K-sized sets in a workgroup's LDS sums (+ the pixel sum)
    __device__ __forceinline__ float pix(float d) const { return fabsf(d); }
    __device__ __forceinline__ float pix_grad(float d) const { return loss_sign(d); }
    __device__ __forceinline__ float reg_a(float u) const {
        const float au = fabsf(u);
        return au < 1.f ? 0.5f * u * u : au - 0.5f;             // SmoothL1Loss(beta = 1)
    }
    __device__ __forceinline__ float reg_a_grad(float u) const { return fabsf(u) < 1.f ? u : loss_sign(u); }
    // per region in the soft kernels, where no pix_grad shares the sign: the saturated branch never sees 0, so the
    // two-valued sign is enough there, and cheaper
    __device__ __forceinline__ float reg_a_grad_soft(float u) const { return fabsf(u) < 1.f ? u : (u > 0.f ? 1.f : -1.f); }
};

struct LossCrit {
    float thr, a2, a1, a0;
};
__device__ __forceinline__ float loss_crit(float u, const LossCrit& c) {
    const float au = fabsf(u);
    return au < c.thr ? c.a2 * u * u : c.a1 * au + c.a0;
}
__device__ __forceinline__ float loss_crit_grad(float u, const LossCrit& c) {
    return fabsf(u) < c.thr ? (2.f * c.a2) * u : c.a1 * loss_sign(u);
}
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

struct LossCodes {                                               // the kernel argument of LossArgs
    int pixel;
    LossCrit qa, qb;
};
template <bool B>
struct LossArgs : LossCodes {
    static constexpr bool HAS_B = B;
    static constexpr int LDS_SETS = 3;
    __device__ __forceinline__ float pix(float d) const { return loss_pix(d, pixel); }
    __device__ __forceinline__ float pix_grad(float d) const { return loss_pix_grad(d, pixel); }
    __device__ __forceinline__ float reg_a(float u) const { return loss_crit(u, qa); }
    __device__ __forceinline__ float reg_a_grad(float u) const { return loss_crit_grad(u, qa); }
    __device__ __forceinline__ float reg_a_grad_soft(float u) const { return loss_crit_grad(u, qa); }
    __device__ __forceinline__ float reg_b(float u) const { return loss_crit(u, qb); }
    __device__ __forceinline__ float reg_b_grad(float u) const { return loss_crit_grad(u, qb); }
};

// the sums layout is the policy's: 2K+1 entries, 3K+1 with the B numerators
template <class P>
constexpr int loss_nsums(int K) { return (P::HAS_B ? 3 : 2) * K + 1; }

// ---- one-hot masks -------------------------------------------------------------------------------------------------------
template <class P>
__global__ void __launch_bounds__(256) k_loss_sums(const float* __restrict__ sr, const float* __restrict__ hr,
                                                   const unsigned char* __restrict__ region, float* __restrict__ sums,
                                                   int B, int C, int h, int w, int s, int K, P p) {
    __shared__ float red[P::LDS_SETS * LOSS_MAXK + 2];
    const int nsums = loss_nsums<P>(K);
    for (int i = threadIdx.x; i < nsums; i += 256) red[i] = 0.f;
    __syncthreads();
    const int W = w * s, H = h * s;
    // one thread = one LR-pixel-wide run of s HR pixels in one row of one channel: a single region
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
            px += p.pix(d);
            na += p.reg_a(d);
            if constexpr (P::HAS_B) nb += p.reg_b(d);
        }
        if (k < K) {
            atomicAdd(&red[k], na);
            atomicAdd(&red[K + k], (float)s);
            if (P::HAS_B) atomicAdd(&red[2 * K + 1 + k], nb);
        }
    }
    for (int off = 32; off > 0; off >>= 1) px += __shfl_down(px, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], px);
    __syncthreads();
    for (int i = threadIdx.x; i < nsums; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * pix'(d) + dsums[region] * A'(d) (+ dsums[2K+1+region] * B'(d))
template <class P>
__global__ void __launch_bounds__(256) k_loss_bwd(const float* __restrict__ sr, const float* __restrict__ hr,
                                                  const unsigned char* __restrict__ region,
                                                  const float* __restrict__ dsums, float* __restrict__ dsr, int B,
                                                  int C, int h, int w, int s, int K, P p) {
    const int W = w * s, H = h * s;
    const size_t n = (size_t)B * C * H * W;
    const float dpx = dsums[2 * K];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int X = (int)(i % W), Y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H * C));
        const int k = region[((size_t)b * h + Y / s) * w + X / s];
        const float d = sr[i] - hr[i];
        float g = dpx * p.pix_grad(d);
        if (k < K) {
            g += dsums[k] * p.reg_a_grad(d);
            if constexpr (P::HAS_B) g += dsums[2 * K + 1 + k] * p.reg_b_grad(d);
        }
        dsr[i] = g;
    }
}

// ---- soft masks ----------------------------------------------------------------------------------------------------------
template <int K, class P>
__device__ __forceinline__ void loss_soft_px(float d, const float (&m)[K], float (&na)[K], float (&nb)[P::HAS_B ? K : 1],
                                             float& px, const P& p) {
    px += p.pix(d);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d;
        na[k] += p.reg_a(u);
        if constexpr (P::HAS_B) nb[k] += p.reg_b(u);
    }
}

// fa / fb: dsums[k] * M_k and dsums[2K+1+k] * M_k
template <int K, class P>
__device__ __forceinline__ float loss_soft_px_bwd(float d, float dpx, const float (&m)[K], const float (&fa)[K],
                                                  const float (&fb)[P::HAS_B ? K : 1], const P& p) {
    float g = dpx * p.pix_grad(d);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float u = m[k] * d;
        g += fa[k] * p.reg_a_grad_soft(u);
        if constexpr (P::HAS_B) g += fb[k] * p.reg_b_grad(u);
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
template <int K, bool VEC, class P>
__global__ void __launch_bounds__(256) k_loss_sums_soft(const float* __restrict__ sr, const float* __restrict__ hr,
                                                        const float* __restrict__ mask, float* __restrict__ sums, int B,
                                                        int C, int h, int w, int s, P p) {
    constexpr int KB = P::HAS_B ? K : 1;
    constexpr int NSUMS = loss_nsums<P>(K);
    __shared__ float red[P::LDS_SETS * LOSS_MAXK + 1];
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
                    for (int i = 0; i < 4; ++i) loss_soft_px<K, P>(d[i], m, na, nb, px, p);
                }
            } else {
                for (int j = 0; j < s; ++j) loss_soft_px<K, P>(ps[j] - ph[j], m, na, nb, px, p);
            }
        }
    }
    // wave reduction, then ONE LDS atomic per wave and sum, then one global atomic per workgroup and sum
    const float area_scale = (float)C * (float)s * (float)s;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float a = na[k], b = area[k], c = nb[P::HAS_B ? k : 0];
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
            if (P::HAS_B) c += __shfl_down(c, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&red[k], a);
            atomicAdd(&red[K + k], b * area_scale);
            if (P::HAS_B) atomicAdd(&red[2 * K + 1 + k], c);
        }
    }
    for (int off = 32; off > 0; off >>= 1) px += __shfl_down(px, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[2 * K], px);
    __syncthreads();
    for (int i = threadIdx.x; i < NSUMS; i += 256) atomicAdd(&sums[i], red[i]);
}

// dsr = dsums[2K] * pix'(d) + sum_k M_k * (dsums[k] * A'(M_k d) + dsums[2K+1+k] * B'(M_k d))
template <int K, bool VEC, class P>
__global__ void __launch_bounds__(256) k_loss_bwd_soft(const float* __restrict__ sr, const float* __restrict__ hr,
                                                       const float* __restrict__ mask, const float* __restrict__ dsums,
                                                       float* __restrict__ dsr, int B, int C, int h, int w, int s, P p) {
    constexpr int KB = P::HAS_B ? K : 1;
    const size_t plane = (size_t)h * s * w * s;
    const size_t nruns = (size_t)B * h * s * w;
    float da[K], db[KB], m[K], fa[K], fb[KB];
#pragma unroll
    for (int k = 0; k < K; ++k) da[k] = dsums[k];
#pragma unroll
    for (int k = 0; k < KB; ++k) db[k] = P::HAS_B ? dsums[2 * K + 1 + k] : 0.f;
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
                    for (int i = 0; i < 4; ++i) g[i] = loss_soft_px_bwd<K, P>(d[i], dpx, m, fa, fb, p);
                    *reinterpret_cast<f32x4*>(pd + j) = g;
                }
            } else {
                for (int j = 0; j < s; ++j) pd[j] = loss_soft_px_bwd<K, P>(ps[j] - ph[j], dpx, m, fa, fb, p);
            }
        }
    }
}

// ---- entry points --------------------------------------------------------------------------------------------------------
// one instantiation per K (1 .. LOSS_MAXK), load width and policy
#define LOSS_CASE(KK, KERNEL, ...)                                                                                   \
    case KK:                                                                                                         \
        if (vec) DASR_LAUNCH((KERNEL<KK, true, P>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);   \
        else DASR_LAUNCH((KERNEL<KK, false, P>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, __VA_ARGS__);      \
        break;
#define LOSS_DISPATCH(KERNEL, ...)                                                                                    \
    switch (K) {                                                                                                      \
        LOSS_CASE(1, KERNEL, __VA_ARGS__) LOSS_CASE(2, KERNEL, __VA_ARGS__) LOSS_CASE(3, KERNEL, __VA_ARGS__)         \
        LOSS_CASE(4, KERNEL, __VA_ARGS__) LOSS_CASE(5, KERNEL, __VA_ARGS__) LOSS_CASE(6, KERNEL, __VA_ARGS__)         \
        LOSS_CASE(7, KERNEL, __VA_ARGS__) LOSS_CASE(8, KERNEL, __VA_ARGS__) LOSS_CASE(9, KERNEL, __VA_ARGS__)         \
        LOSS_CASE(10, KERNEL, __VA_ARGS__) LOSS_CASE(11, KERNEL, __VA_ARGS__) LOSS_CASE(12, KERNEL, __VA_ARGS__)      \
        LOSS_CASE(13, KERNEL, __VA_ARGS__) LOSS_CASE(14, KERNEL, __VA_ARGS__) LOSS_CASE(15, KERNEL, __VA_ARGS__)      \
        LOSS_CASE(16, KERNEL, __VA_ARGS__)                                                                            \
        default: return DASR_E_UNSUPPORTED;                                                                           \
    }

// What all eight entry points do.  AUX: unsigned char (region bytes) or float (soft masks).  BWD: ``out`` is dsr and
// ``dsums`` is read; otherwise ``out`` is the sums vector, cleared here, and ``dsums`` is not looked at.  ``known``: the
// criterion codes name something the family computes - anything else is refused before a launch.
template <bool BWD, class AUX, class P>
static int loss_launch(const float* sr, const float* hr, const AUX* aux, const float* dsums, float* out, int B, int C,
                       int h, int w, int s, int K, bool known, const P& p, void* stream) {
    DASR_CHECK_PTR(sr); DASR_CHECK_PTR(hr); DASR_CHECK_PTR(aux); DASR_CHECK_PTR(out);
    if (BWD) DASR_CHECK_PTR(dsums);
    DASR_CHECK_SHAPE(B > 0 && C > 0 && h > 0 && w > 0 && s > 0 && K > 0);
    if (K > LOSS_MAXK || !known) return DASR_E_UNSUPPORTED;
    if (!BWD) {
        hipError_t e = hipMemsetAsync(out, 0, sizeof(float) * loss_nsums<P>(K), (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if constexpr (std::is_same<AUX, unsigned char>::value) {
        const size_t nruns = (size_t)B * C * h * s * w;
        if constexpr (BWD)
            DASR_LAUNCH((k_loss_bwd<P>), dim3(dasr_ew_grid(nruns * s)), dim3(256), 0, stream, sr, hr, aux, dsums, out, B, C, h, w, s, K, p);
        else
            DASR_LAUNCH((k_loss_sums<P>), dim3(dasr_ew_grid(nruns)), dim3(256), 0, stream, sr, hr, aux, out, B, C, h, w, s, K, p);
    } else {
        const size_t nruns = (size_t)B * h * s * w;
        const bool vec = s % 4 == 0 && ((((uintptr_t)sr | (uintptr_t)hr | (BWD ? (uintptr_t)out : 0)) & 15) == 0);
        if constexpr (BWD) {
            LOSS_DISPATCH(k_loss_bwd_soft, sr, hr, aux, dsums, out, B, C, h, w, s, p)
        } else {
            LOSS_DISPATCH(k_loss_sums_soft, sr, hr, aux, out, B, C, h, w, s, p)
        }
    }
    DASR_RETURN_LAUNCH_STATUS();
}

static inline bool loss_region_crit(int code, LossCrit& c) {
    if (code == DASR_CRIT_L1) c = LossCrit{0.f, 0.f, 1.f, 0.f};
    else if (code == DASR_CRIT_L2) c = LossCrit{__builtin_inff(), 1.f, 0.f, 0.f};
    else if (code == DASR_CRIT_SMOOTHL1) c = LossCrit{1.f, 0.5f, 1.f, -0.5f};
    else return false;
    return true;
}

// codes -> coefficients -> LossArgs<with or without B>
template <bool BWD, class AUX>
static int loss_launch_crit(const float* sr, const float* hr, const AUX* aux, const float* dsums, float* out, int B, int C,
                            int h, int w, int s, int K, int pixel_crit, int crit_a, int crit_b, void* stream) {
    LossCodes q{pixel_crit, LossCrit{0.f, 0.f, 0.f, 0.f}, LossCrit{0.f, 0.f, 0.f, 0.f}};
    const bool has_b = crit_b != DASR_CRIT_NONE;
    const bool known = (pixel_crit == DASR_CRIT_L1 || pixel_crit == DASR_CRIT_L2 || pixel_crit == DASR_CRIT_CB) &&
                       loss_region_crit(crit_a, q.qa) && (!has_b || loss_region_crit(crit_b, q.qb));
    if (has_b) return loss_launch<BWD>(sr, hr, aux, dsums, out, B, C, h, w, s, K, known, LossArgs<true>{q}, stream);
    return loss_launch<BWD>(sr, hr, aux, dsums, out, B, C, h, w, s, K, known, LossArgs<false>{q}, stream);
}

extern "C" int dasr_loss_sums(const float* sr, const float* hr, const unsigned char* region, float* sums, int B, int C,
                              int h, int w, int scale, int K, void* stream) {
    return loss_launch<false>(sr, hr, region, nullptr, sums, B, C, h, w, scale, K, true, LossFixed{}, stream);
}

extern "C" int dasr_loss_bwd(const float* sr, const float* hr, const unsigned char* region, const float* dsums,
                             float* dsr, int B, int C, int h, int w, int scale, int K, void* stream) {
    return loss_launch<true>(sr, hr, region, dsums, dsr, B, C, h, w, scale, K, true, LossFixed{}, stream);
}

extern "C" int dasr_loss_sums_soft(const float* sr, const float* hr, const float* mask, float* sums, int B, int C, int h,
                                   int w, int scale, int K, void* stream) {
    return loss_launch<false>(sr, hr, mask, nullptr, sums, B, C, h, w, scale, K, true, LossFixed{}, stream);
}

extern "C" int dasr_loss_bwd_soft(const float* sr, const float* hr, const float* mask, const float* dsums, float* dsr,
                                  int B, int C, int h, int w, int scale, int K, void* stream) {
    return loss_launch<true>(sr, hr, mask, dsums, dsr, B, C, h, w, scale, K, true, LossFixed{}, stream);
}

extern "C" int dasr_loss_sums_crit(const float* sr, const float* hr, const unsigned char* region, float* sums, int B,
                                   int C, int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b,
                                   void* stream) {
    return loss_launch_crit<false>(sr, hr, region, nullptr, sums, B, C, h, w, scale, K, pixel_crit, crit_a, crit_b, stream);
}

extern "C" int dasr_loss_bwd_crit(const float* sr, const float* hr, const unsigned char* region, const float* dsums,
                                  float* dsr, int B, int C, int h, int w, int scale, int K, int pixel_crit, int crit_a,
                                  int crit_b, void* stream) {
    return loss_launch_crit<true>(sr, hr, region, dsums, dsr, B, C, h, w, scale, K, pixel_crit, crit_a, crit_b, stream);
}

extern "C" int dasr_loss_sums_soft_crit(const float* sr, const float* hr, const float* mask, float* sums, int B, int C,
                                        int h, int w, int scale, int K, int pixel_crit, int crit_a, int crit_b,
                                        void* stream) {
    return loss_launch_crit<false>(sr, hr, mask, nullptr, sums, B, C, h, w, scale, K, pixel_crit, crit_a, crit_b, stream);
}

extern "C" int dasr_loss_bwd_soft_crit(const float* sr, const float* hr, const float* mask, const float* dsums,
                                       float* dsr, int B, int C, int h, int w, int scale, int K, int pixel_crit,
                                       int crit_a, int crit_b, void* stream) {
    return loss_launch_crit<true>(sr, hr, mask, dsums, dsr, B, C, h, w, scale, K, pixel_crit, crit_a, crit_b, stream);
}
