// prep.hip — device-side input preparation: the reference's getDepthMask binning
// (codes/data/LQGTker_Depth_dataset.py:204-225) from the depth map straight to the region byte the one-hot SEAN
// kernels read, and optionally to the K float planes the module API takes.  Only the depth map crosses PCIe.
//
// Rule restated (float32 arithmetic exactly as torch evaluates it on 0-dim float32 tensors, no FMA contraction):
//   lo, hi   = min, max of the sample's depth map            (depthFixedRange: lo = 0, hi = 1)
//   interval = (hi - lo) / K
//   bin i    = [lo + interval*i, lo + interval*(i+1))         i = 0..K-1
// A pixel equal to the maximum (or outside [0,1) in fixed-range mode) belongs to no bin: region byte = K, all planes 0.
// In fixed-range mode the reference computes the edges in Python doubles (0 + 0.1*i) and torch compares the float32
// map against them rounded to float32; the edges are passed in from the host for that mode.
#include "dasr_common.h"

#if DASR_DEVICE_BUILD
__device__ __forceinline__ float prep_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float prep_add(float a, float b) { return __fadd_rn(a, b); }
#else
static inline float prep_mul(float a, float b) { volatile float r = a * b; return r; }
static inline float prep_add(float a, float b) { volatile float r = a + b; return r; }
#endif
// IEEE division, rounded on its own (the soft rule below; a float32 numpy restatement gives the same bits)
#if DASR_DEVICE_BUILD
__device__ __forceinline__ float prep_div(float a, float b) { return __fdiv_rn(a, b); }
#else
static inline float prep_div(float a, float b) { volatile float r = a / b; return r; }
#endif

#define PREP_MAXK 16
#define PREP_CHUNK 4096

// partial min / max of chunk blockIdx.x of sample blockIdx.y -> ws[(b*nchunk + chunk)*2 + {0,1}]
__global__ void __launch_bounds__(256) k_depth_minmax(const float* __restrict__ depth, float* __restrict__ ws, int HW,
                                                      int nchunk) {
    __shared__ float slo[4], shi[4];
    const int b = blockIdx.y;
    const float* d = depth + (size_t)b * HW;
    const int per = (HW + nchunk - 1) / nchunk;
    const int p0 = blockIdx.x * per, p1 = p0 + per < HW ? p0 + per : HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        const float v = d[p];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, 64));
        hi = fmaxf(hi, __shfl_down(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = lo; shi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[((size_t)b * nchunk + blockIdx.x) * 2 + 0] = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
        ws[((size_t)b * nchunk + blockIdx.x) * 2 + 1] = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    }
}

// region byte (and the K float planes) of every pixel
__global__ void __launch_bounds__(256) k_depth_bins(const float* __restrict__ depth, const float* __restrict__ ws,
                                                    const float* __restrict__ fixed_edges, float* __restrict__ masks,
                                                    unsigned char* __restrict__ region, int HW, int K, int nchunk) {
    __shared__ float edge[PREP_MAXK + 1];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        if (fixed_edges) {
            for (int i = 0; i <= K; ++i) edge[i] = fixed_edges[i];
        } else {
            float lo = INFINITY, hi = -INFINITY;
            for (int c = 0; c < nchunk; ++c) {
                lo = fminf(lo, ws[((size_t)b * nchunk + c) * 2 + 0]);
                hi = fmaxf(hi, ws[((size_t)b * nchunk + c) * 2 + 1]);
            }
            const float interval = prep_add(hi, -lo) / (float)K;          // IEEE division, like torch
            for (int i = 0; i <= K; ++i) edge[i] = prep_add(lo, prep_mul(interval, (float)i));
        }
    }
    __syncthreads();
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const float v = depth[(size_t)b * HW + p];
        int idx = K;
        for (int i = 0; i < K; ++i)
            if (v >= edge[i] && v < edge[i + 1]) idx = i;
        if (region) region[(size_t)b * HW + p] = (unsigned char)idx;
        if (masks)
            for (int i = 0; i < K; ++i) masks[((size_t)b * K + i) * HW + p] = i == idx ? 1.f : 0.f;
    }
}

// ---- soft (hat-function) membership ------------------------------------------------------------------------------------
// The same range and interval as above, but every pixel is shared between the bin it falls into and the nearer neighbour:
//   u = clamp((v - lo) / interval, 0, K);  k = min(floor(u), K-1);  r = u - k
//   r < 0.5:  n = k - 1, s = 0.5 - r / width        else:  n = k + 1, s = 0.5 - (1 - r) / width
//   s = max(s, 0), 0 where n is no plane;  plane[k] = 1 - s, plane[n] = s, every other plane 0
// width = 1 interpolates linearly between bin centres; a smaller width narrows the blend to a band of width * interval
// around each interior edge; width -> 0 tends to the one-hot rule.  At most two planes are non-zero and they sum to 1; each
// plane is Lipschitz in v with constant 1 / (interval * width).  Unlike the one-hot rule, which leaves the maximum pixel
// in no bin, the maximum belongs to plane K-1 (u == K, r == 1); a constant map (interval not > 0) is all plane 0.
// Every operation is rounded on its own in float32 (prep_add / prep_mul / prep_div).  NaN depth: unspecified.
struct prep_soft_t { int k, n; float wk, wn; };

__device__ __forceinline__ prep_soft_t prep_soft(float v, float lo, float interval, int K, float width) {
    prep_soft_t o;
    if (!(interval > 0.f)) { o.k = 0; o.n = -1; o.wk = 1.f; o.wn = 0.f; return o; }
    float u = prep_div(prep_add(v, -lo), interval);
    u = fminf(fmaxf(u, 0.f), (float)K);
    int k = (int)floorf(u);
    k = k < K - 1 ? k : K - 1;
    const float r = prep_add(u, -(float)k);
    int n;
    float s;
    if (r < 0.5f) {
        n = k - 1;
        s = prep_add(0.5f, -prep_div(r, width));
    } else {
        n = k + 1;
        s = prep_add(0.5f, -prep_div(prep_add(1.f, -r), width));
    }
    s = fmaxf(s, 0.f);
    if (n < 0 || n >= K) s = 0.f;
    o.k = k; o.n = n; o.wk = prep_add(1.f, -s); o.wn = s;
    return o;
}

// all K planes in one launch; a lane owns four consecutive pixels and writes, plane by plane, one 16-byte store where the
// four are inside the map and their address is 16-byte aligned, scalar stores otherwise (the tail of a map whose size is
// no multiple of 4, planes that start off the 16-byte grid).  Every element of masks is written, zeros included.
// PAIR: the same launch also writes the pixel's pair encoding (include/dasr.h) - pair_k = k as a plain byte store, like the
// region bytes of k_depth_bins, and pair_s = -s where the neighbour is k - 1 and s > 0, else s (so a pixel without a second
// plane holds +0.0, never -0.0) - and masks may be NULL, in which case the planes are not written.
template <bool PAIR>
__global__ void __launch_bounds__(256) k_depth_soft(const float* __restrict__ depth, const float* __restrict__ ws,
                                                    float* __restrict__ masks, unsigned char* __restrict__ pair_k,
                                                    float* __restrict__ pair_s, int HW, int K, int nchunk, float width,
                                                    int fixed_range) {
    __shared__ float s_range[2];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) {
        float lo = 0.f, hi = 1.f;
        if (!fixed_range) {
            lo = INFINITY, hi = -INFINITY;
            for (int c = 0; c < nchunk; ++c) {
                lo = fminf(lo, ws[((size_t)b * nchunk + c) * 2 + 0]);
                hi = fmaxf(hi, ws[((size_t)b * nchunk + c) * 2 + 1]);
            }
        }
        s_range[0] = lo;
        s_range[1] = prep_div(prep_add(hi, -lo), (float)K);
    }
    __syncthreads();
    const float lo = s_range[0], interval = s_range[1];
    const float* d = depth + (size_t)b * HW;
    float* m = masks + (size_t)b * K * HW;
    const int nquad = (int)(((size_t)HW + 3) >> 2);
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nquad; q += gridDim.x * 256) {
        const size_t p0 = (size_t)q * 4;
        const bool full = p0 + 4 <= (size_t)HW;
        const int cnt = full ? 4 : (int)((size_t)HW - p0);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (full && ((uintptr_t)(d + p0) & 15) == 0) {
            const float4 t = *(const float4*)(d + p0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) v[j] = d[p0 + j];
        }
        prep_soft_t e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = prep_soft(v[j], lo, interval, K, width);
        if (PAIR) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (e[j].n < e[j].k && e[j].wn > 0.f) ? -e[j].wn : e[j].wn;
            unsigned char* dk = pair_k + (size_t)b * HW + p0;
            float* ds = pair_s + (size_t)b * HW + p0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) dk[j] = (unsigned char)e[j].k;
            if (full && ((uintptr_t)ds & 15) == 0) {
                *(float4*)ds = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) ds[j] = o[j];
            }
            if (masks == nullptr) continue;
        }
        for (int i = 0; i < K; ++i) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = i == e[j].k ? e[j].wk : (i == e[j].n ? e[j].wn : 0.f);
            float* dst = m + (size_t)i * HW + p0;
            if (full && ((uintptr_t)dst & 15) == 0) {
                *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) dst[j] = o[j];
            }
        }
    }
}

static int prep_nchunk(int HW) {
    int n = (HW + PREP_CHUNK - 1) / PREP_CHUNK;
    return n > 64 ? 64 : (n < 1 ? 1 : n);
}

extern "C" size_t dasr_depth_to_masks_workspace(int B, int HW) {
    if (B <= 0 || HW <= 0) return 0;
    return sizeof(float) * 2 * (size_t)B * prep_nchunk(HW);
}

extern "C" int dasr_depth_to_masks(const float* depth, const float* fixed_edges, float* masks, unsigned char* region,
                                   void* workspace, size_t workspace_bytes, int B, int HW, int K, void* stream) {
    DASR_CHECK_PTR(depth); DASR_CHECK_PTR(workspace);
    if (masks == nullptr && region == nullptr) return DASR_E_NULL;
    DASR_CHECK_SHAPE(B > 0 && HW > 0 && K > 0);
    if (K > PREP_MAXK) return DASR_E_UNSUPPORTED;
    if (workspace_bytes < dasr_depth_to_masks_workspace(B, HW)) return DASR_E_WORKSPACE;
    const int nchunk = prep_nchunk(HW);
    if (!fixed_edges)
        DASR_LAUNCH(k_depth_minmax, dim3(nchunk, B), dim3(256), 0, stream, depth, (float*)workspace, HW, nchunk);
    unsigned gx = dasr_cdiv((size_t)HW, 256);
    if (gx > 1024) gx = 1024;
    DASR_LAUNCH(k_depth_bins, dim3(gx, B), dim3(256), 0, stream, depth, (const float*)workspace, fixed_edges, masks, region,
                HW, K, nchunk);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" size_t dasr_depth_to_masks_soft_workspace(int B, int HW) { return dasr_depth_to_masks_workspace(B, HW); }

template <bool PAIR>
static int depth_soft_impl(const float* depth, float* masks, unsigned char* pair_k, float* pair_s, void* workspace,
                           size_t workspace_bytes, int B, int HW, int K, float width, int fixed_range, void* stream) {
    DASR_CHECK_PTR(depth); DASR_CHECK_PTR(workspace);
    if (PAIR) { DASR_CHECK_PTR(pair_k); DASR_CHECK_PTR(pair_s); }
    else DASR_CHECK_PTR(masks);
    DASR_CHECK_SHAPE(B > 0 && HW > 0 && K > 0);
    if (K > PREP_MAXK) return DASR_E_UNSUPPORTED;
    DASR_CHECK_SHAPE(width > 0.f && width <= 1.f);                        // false for NaN too
    if (workspace_bytes < dasr_depth_to_masks_soft_workspace(B, HW)) return DASR_E_WORKSPACE;
    const int nchunk = prep_nchunk(HW);
    if (!fixed_range)
        DASR_LAUNCH(k_depth_minmax, dim3(nchunk, B), dim3(256), 0, stream, depth, (float*)workspace, HW, nchunk);
    unsigned gx = dasr_cdiv(((size_t)HW + 3) / 4, 256);                   // a lane owns four pixels
    if (gx > 1024) gx = 1024;
    DASR_LAUNCH((k_depth_soft<PAIR>), dim3(gx, B), dim3(256), 0, stream, depth, (const float*)workspace, masks, pair_k, pair_s,
                HW, K, nchunk, width, fixed_range != 0 ? 1 : 0);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_depth_to_masks_soft(const float* depth, float* masks, void* workspace, size_t workspace_bytes, int B,
                                        int HW, int K, float width, int fixed_range, void* stream) {
    return depth_soft_impl<false>(depth, masks, nullptr, nullptr, workspace, workspace_bytes, B, HW, K, width, fixed_range,
                                  stream);
}

extern "C" int dasr_depth_to_masks_soft_pair(const float* depth, float* masks, unsigned char* pair_k, float* pair_s,
                                             void* workspace, size_t workspace_bytes, int B, int HW, int K, float width,
                                             int fixed_range, void* stream) {
    return depth_soft_impl<true>(depth, masks, pair_k, pair_s, workspace, workspace_bytes, B, HW, K, width, fixed_range,
                                 stream);
}
