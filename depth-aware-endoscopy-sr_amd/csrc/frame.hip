// frame.hip — the uint8 edge of video inference: camera frames in, displayable frames out, PSNR sums where the images are.
//
//   dasr_frame_ingest_u8   uint8 [B,H,W,C] (HWC; BGR for C == 3 with swap_rb) -> float NHWC RGB, x / 255 (IEEE division):
//                          img2tensor / read_img of the reference (utils/util.py) without the host float image, the NCHW
//                          transpose and its inverse on the device
//   dasr_frame_emit_u8     float NHWC (conv_output's result, before the clamp) -> uint8 HWC (BGR): torch.clamp
//                          (sftmd_arch.py:950) + tensor2img (utils/util.py:572-590) in one pass
//   dasr_frame_ssd_u8      exact integer sum of squared differences of two uint8 images inside a cropped border: the
//                          numerator of calculate_psnr (utils/util.py:646-653) as train.py:245-262 calls it
//
// All three move bytes.  Ingest and emit treat the whole batch as ONE flat array (H*W*C need not be a multiple of 4, so
// a frame's base is not dword aligned): a wide body of 12-element groups - four 3-channel pixels: 12 bytes on the uint8
// side, three float4 on the fp32 side, so the R<->B swap never crosses a lane - between a scalar head (the elements before
// the first group whose two addresses are both aligned) and a scalar tail.  No atomics: the SSD goes through one 64-bit
// partial per workgroup in the caller's workspace and a second small launch, like pool.hip / loss.hip / prep.hip.
#include "dasr_common.h"

#if DASR_DEVICE_BUILD
__device__ __forceinline__ float frame_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float frame_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float frame_mul(float a, float b) { return __fmul_rn(a, b); }
#else
static inline float frame_div(float a, float b) { volatile float r = a / b; return r; }
static inline float frame_sub(float a, float b) { volatile float r = a - b; return r; }
static inline float frame_mul(float a, float b) { volatile float r = a * b; return r; }
#endif

struct alignas(4) frame_u8x12 { unsigned w[3]; };       // twelve bytes, one dwordx3 access
struct alignas(16) frame_u32x4 { unsigned x, y, z, w; };  // sixteen bytes, one dwordx4 access

#define FRAME_GROUP 12

// source element of destination element e of a 12-element group (both directions: the swap is its own inverse)
template <bool SWAP>
__device__ __forceinline__ constexpr int frame_src(int e) { return SWAP ? e - e % 3 + (2 - e % 3) : e; }

// ---- ingest ----------------------------------------------------------------------------------------------------------
// elements [0, head) and [head + 12 ngroups, n) one per thread iteration, the groups in between one per thread iteration
template <bool SWAP>
__global__ void __launch_bounds__(256) k_frame_ingest(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                      size_t head, size_t ngroups, size_t n) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthr = (size_t)gridDim.x * 256;
    const size_t body_end = head + FRAME_GROUP * ngroups;
    const size_t nscalar = head + (n - body_end);
    for (size_t i = tid; i < nscalar; i += nthr) {
        const size_t e = i < head ? i : body_end + (i - head);
        const size_t s = SWAP ? e - e % 3 + (2 - e % 3) : e;
        dst[e] = frame_div((float)src[s], 255.0f);
    }
    for (size_t g = tid; g < ngroups; g += nthr) {
        const frame_u8x12 in = *(const frame_u8x12*)(src + head + FRAME_GROUP * g);
        float v[FRAME_GROUP];
#pragma unroll
        for (int e = 0; e < FRAME_GROUP; ++e) {
            const int s = frame_src<SWAP>(e);
            v[e] = frame_div((float)((in.w[s >> 2] >> (8 * (s & 3))) & 0xffu), 255.0f);
        }
        float4* out = (float4*)(dst + head + FRAME_GROUP * g);
        out[0] = make_float4(v[0], v[1], v[2], v[3]);
        out[1] = make_float4(v[4], v[5], v[6], v[7]);
        out[2] = make_float4(v[8], v[9], v[10], v[11]);
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------
struct frame_emit_par { float net_lo, net_hi, mm_lo, mm_hi, mm_den; };

__device__ __forceinline__ unsigned frame_quant(float y, const frame_emit_par& p) {
    float v = fminf(fmaxf(y, p.net_lo), p.net_hi);            // torch.clamp(out, min, max), sftmd_arch.py:950
    v = fminf(fmaxf(v, p.mm_lo), p.mm_hi);                    // tensor.clamp_(*min_max)
    v = frame_div(frame_sub(v, p.mm_lo), p.mm_den);           // (tensor - min) / (max - min)
    return (unsigned)(int)rintf(frame_mul(v, 255.0f));        // (img * 255.0).round(): ties to even, in fp32
}

template <bool SWAP>
__global__ void __launch_bounds__(256) k_frame_emit(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                    size_t head, size_t ngroups, size_t n, frame_emit_par p) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthr = (size_t)gridDim.x * 256;
    const size_t body_end = head + FRAME_GROUP * ngroups;
    const size_t nscalar = head + (n - body_end);
    for (size_t i = tid; i < nscalar; i += nthr) {
        const size_t e = i < head ? i : body_end + (i - head);
        const size_t s = SWAP ? e - e % 3 + (2 - e % 3) : e;
        dst[e] = (unsigned char)frame_quant(src[s], p);
    }
    for (size_t g = tid; g < ngroups; g += nthr) {
        const float4* in = (const float4*)(src + head + FRAME_GROUP * g);
        const float4 a = in[0], b = in[1], c = in[2];
        const float v[FRAME_GROUP] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        frame_u8x12 out = {{0u, 0u, 0u}};
#pragma unroll
        for (int e = 0; e < FRAME_GROUP; ++e) out.w[e >> 2] |= frame_quant(v[frame_src<SWAP>(e)], p) << (8 * (e & 3));
        *(frame_u8x12*)(dst + head + FRAME_GROUP * g) = out;
    }
}

// The first group boundary at which the uint8 side is dword aligned and the fp32 side 16-byte aligned.  `unit`: elements
// that may not be split between head and body (3 with the channel swap, else 1).  No such boundary: everything is "head".
static size_t frame_head(const void* u8, const void* f32, size_t n, size_t unit) {
    for (size_t h = 0; h < 16 * unit && h <= n; h += unit)
        if (((uintptr_t)u8 + h) % 4 == 0 && ((uintptr_t)f32 + 4 * h) % 16 == 0) return h;
    return n;
}

extern "C" int dasr_frame_ingest_u8(const unsigned char* frames, float* x_nhwc, int B, int H, int W, int C, int swap_rb,
                                    void* stream) {
    DASR_CHECK_PTR(frames); DASR_CHECK_PTR(x_nhwc);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && C > 0);
    const bool swap = swap_rb && C == 3;
    const size_t n = (size_t)B * H * W * C;
    const size_t head = frame_head(frames, x_nhwc, n, swap ? 3 : 1);
    const size_t ngroups = (n - head) / FRAME_GROUP;
    const size_t work = ngroups > n - FRAME_GROUP * ngroups ? ngroups : n - FRAME_GROUP * ngroups;
    if (swap)
        DASR_LAUNCH(k_frame_ingest<true>, dim3(dasr_ew_grid(work)), dim3(256), 0, stream, frames, x_nhwc, head, ngroups, n);
    else
        DASR_LAUNCH(k_frame_ingest<false>, dim3(dasr_ew_grid(work)), dim3(256), 0, stream, frames, x_nhwc, head, ngroups, n);
    DASR_RETURN_LAUNCH_STATUS();
}

extern "C" int dasr_frame_emit_u8(const float* y_nhwc, unsigned char* frames, int B, int H, int W, int C, float net_lo,
                                  float net_hi, double mm_lo, double mm_hi, int swap_rb, void* stream) {
    DASR_CHECK_PTR(y_nhwc); DASR_CHECK_PTR(frames);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && C > 0 && mm_hi > mm_lo);
    if (C != 1 && C != 3) return DASR_E_UNSUPPORTED;
    // tensor2img takes min_max as Python numbers: the difference is formed in double and torch rounds each scalar
    // operand to float32 once
    const frame_emit_par p = {net_lo, net_hi, (float)mm_lo, (float)mm_hi, (float)(mm_hi - mm_lo)};
    const bool swap = swap_rb && C == 3;
    const size_t n = (size_t)B * H * W * C;
    const size_t head = frame_head(frames, y_nhwc, n, swap ? 3 : 1);
    const size_t ngroups = (n - head) / FRAME_GROUP;
    const size_t work = ngroups > n - FRAME_GROUP * ngroups ? ngroups : n - FRAME_GROUP * ngroups;
    if (swap)
        DASR_LAUNCH(k_frame_emit<true>, dim3(dasr_ew_grid(work)), dim3(256), 0, stream, y_nhwc, frames, head, ngroups, n, p);
    else
        DASR_LAUNCH(k_frame_emit<false>, dim3(dasr_ew_grid(work)), dim3(256), 0, stream, y_nhwc, frames, head, ngroups, n, p);
    DASR_RETURN_LAUNCH_STATUS();
}

// ---- sum of squared differences ----------------------------------------------------------------------------------------
#define SSD_MAX_CHUNKS 256
// 255^2 * 66051 < 2^32: a thread's 32-bit sum is exact over that many samples.  A thread takes every 256th 16-byte piece of
// ONE row (and at most one of its unaligned end bytes) before it adds into its 64-bit sum: rowlen / 256 + 17 samples.
#define SSD_MAX_ROW ((size_t)256 * 66000)

__device__ __forceinline__ unsigned ssd_word(unsigned a, unsigned b) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((a >> (8 * k)) & 0xffu) - (int)((b >> (8 * k)) & 0xffu);
        s += (unsigned)(d * d);
    }
    return s;
}

// workgroup blockIdx.x of frame blockIdx.y: interior rows chunk, chunk + nchunk, ... -> part[b * nchunk + chunk]
__global__ void __launch_bounds__(256) k_frame_ssd(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                   unsigned long long* __restrict__ part, int H, int W, int C, int crop,
                                                   int nchunk) {
    __shared__ unsigned long long s_part[4];
    const int f = blockIdx.y;
    const size_t rowlen = (size_t)(W - 2 * crop) * C;
    unsigned long long acc = 0;
    for (int y = crop + blockIdx.x; y < H - crop; y += nchunk) {
        const size_t off = (((size_t)f * H + y) * W + crop) * C;
        const unsigned char* pa = a + off;
        const unsigned char* pb = b + off;
        // 16-byte pieces where both rows allow it, single bytes before and after
        size_t head = (size_t)((16 - ((uintptr_t)pa & 15)) & 15);
        if ((((uintptr_t)pa ^ (uintptr_t)pb) & 15) != 0 || head > rowlen) head = rowlen;
        const size_t nvec = (rowlen - head) / 16;
        const size_t tail0 = head + 16 * nvec;
        unsigned s = 0;
        for (size_t i = threadIdx.x; i < head + (rowlen - tail0); i += 256) {
            const size_t e = i < head ? i : tail0 + (i - head);
            const int d = (int)pa[e] - (int)pb[e];
            s += (unsigned)(d * d);
        }
        const frame_u32x4* va = (const frame_u32x4*)(pa + head);
        const frame_u32x4* vb = (const frame_u32x4*)(pb + head);
        for (size_t i = threadIdx.x; i < nvec; i += 256) {
            const frame_u32x4 x = va[i], z = vb[i];
            s += ssd_word(x.x, z.x) + ssd_word(x.y, z.y) + ssd_word(x.z, z.z) + ssd_word(x.w, z.w);
        }
        acc += s;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)f * nchunk + blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// one wave per frame: the partials in a fixed order (integers: any order gives the same sum)
__global__ void __launch_bounds__(64) k_frame_ssd_final(const unsigned long long* __restrict__ part,
                                                        unsigned long long* __restrict__ out, int nchunk) {
    const int f = blockIdx.x;
    unsigned long long acc = 0;
    for (int c = threadIdx.x; c < nchunk; c += 64) acc += part[(size_t)f * nchunk + c];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (threadIdx.x == 0) out[f] = acc;
}

static int ssd_nchunk(int H, int crop) {
    const int rows = H - 2 * crop;
    return rows > SSD_MAX_CHUNKS ? SSD_MAX_CHUNKS : (rows < 1 ? 1 : rows);
}

extern "C" size_t dasr_frame_ssd_u8_workspace(int B, int H, int W, int C, int crop) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || crop < 0) return 0;
    return sizeof(unsigned long long) * (size_t)B * ssd_nchunk(H, crop);
}

extern "C" int dasr_frame_ssd_u8(const unsigned char* a, const unsigned char* b, unsigned long long* ssd, void* workspace,
                                 size_t workspace_bytes, int B, int H, int W, int C, int crop, void* stream) {
    DASR_CHECK_PTR(a); DASR_CHECK_PTR(b); DASR_CHECK_PTR(ssd); DASR_CHECK_PTR(workspace);
    DASR_CHECK_SHAPE(B > 0 && H > 0 && W > 0 && C > 0 && crop >= 0 && B <= 65535);
    if (2 * (long long)crop >= H || 2 * (long long)crop >= W) return DASR_E_UNSUPPORTED;
    if ((size_t)(W - 2 * crop) * C > SSD_MAX_ROW) return DASR_E_UNSUPPORTED;
    if (workspace_bytes < dasr_frame_ssd_u8_workspace(B, H, W, C, crop)) return DASR_E_WORKSPACE;
    const int nchunk = ssd_nchunk(H, crop);
    DASR_LAUNCH(k_frame_ssd, dim3(nchunk, B), dim3(256), 0, stream, a, b, (unsigned long long*)workspace, H, W, C, crop,
                nchunk);
    DASR_LAUNCH(k_frame_ssd_final, dim3(B), dim3(64), 0, stream, (const unsigned long long*)workspace, ssd, nchunk);
    DASR_RETURN_LAUNCH_STATUS();
}
