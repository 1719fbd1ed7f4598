// Device-side input pipeline: what MonoDataset.preprocess does with PIL on 24 host workers per GPU
// (mono/datasets/mono_dataset.py:126-171,417-431) runs here on the raw uint8 frames after ONE pinned async upload:
//   resample   : PIL Image.resize(..., ANTIALIAS == LANCZOS) on 8-bit images, bit-exact: Pillow's two-pass separable
//                convolution with 22-bit fixed-point coefficients and a uint8 intermediate (libImaging/Resample.c; the
//                coefficient tables are built on the host exactly like precompute_coeffs / normalize_coeffs_8bpc)
//   to_tensor  : HWC uint8 -> CHW float / 255 (fused into the vertical pass)
//   ColorJitter: brightness / contrast / saturation / hue in torchvision's tensor arithmetic, in a random order
//   topview    : L conversion, binarise, NEAREST resize to H/4, {0,1} float  (process_topview)
//   flip       : MonoDataset.__getitem__'s do_flip (transpose(FLIP_LEFT_RIGHT) of every raw image / label before any resize), per
//                item from a device flag table: jp_resample_h_u8_flip / jp_u8_to_tensor_flip / jp_topview_u8_flip read a flagged
//                item mirrored; without flags they write what their plain counterparts write
//   batched ColorJitter: jp_color_jitter_batched, N images with N parameter records in two launches, the gray mean of the
//                contrast op folded in a fixed order (no atomics); the per-op kernel and the batched ones share the ops' code
// Third-party semantics (Pillow, torchvision) are restated from their published algorithms; Pillow IS importable in
// the build image, so the resampler is pinned against it (tests/golden/preprocess.npz).
#include "jp_common.h"
#include <algorithm>

namespace {
constexpr int TPB = 256;
constexpr int PBITS = 22;    // PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clip8(int v) {
    v >>= PBITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// horizontal: src (N*H rows, W, C) u8 -> dst (N*H rows, OW, C) u8
__global__ __launch_bounds__(TPB) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const int* __restrict__ bounds, const int* __restrict__ kk,
                                                         long rows, int W, int OW, int C, int ksize) {
    const long total = rows * OW * C;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % C);
        const long t = i / C;
        const int ox = (int)(t % OW);
        const long row = t / OW;
        const int xmin = bounds[2 * ox], xmax = bounds[2 * ox + 1];
        const int* k = kk + (long)ox * ksize;
        const uint8_t* sp = src + (row * W + xmin) * C + c;
        int ss = 1 << (PBITS - 1);
        for (int x = 0; x < xmax; ++x) ss += (int)sp[(long)x * C] * k[x];
        dst[i] = (uint8_t)clip8(ss);
    }
}

// vertical: src (N, H, OW, C) u8 -> out_u8 (N, OH, OW, C) and / or out_f (N, C, OH, OW) = value / 255
__global__ __launch_bounds__(TPB) void resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out_u8,
                                                         float* __restrict__ out_f, const int* __restrict__ bounds,
                                                         const int* __restrict__ kk, int N, int H, int OH, int OW, int C,
                                                         int ksize) {
    const long total = (long)N * OH * OW * C;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % C);
        long t = i / C;
        const int ox = (int)(t % OW);
        t /= OW;
        const int oy = (int)(t % OH);
        const int n = (int)(t / OH);
        const int ymin = bounds[2 * oy], ymax = bounds[2 * oy + 1];
        const int* k = kk + (long)oy * ksize;
        const uint8_t* sp = src + (((long)n * H + ymin) * OW + ox) * C + c;
        int ss = 1 << (PBITS - 1);
        for (int y = 0; y < ymax; ++y) ss += (int)sp[(long)y * OW * C] * k[y];
        const int v = clip8(ss);
        if (out_u8) out_u8[i] = (uint8_t)v;
        if (out_f) out_f[(((long)n * C + c) * OH + oy) * OW + ox] = (float)v / 255.f;      // transforms.ToTensor
    }
}

// HWC u8 -> CHW float / 255 (ToTensor without a resize)
__global__ __launch_bounds__(TPB) void to_tensor_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int N, int H,
                                                        int W, int C) {
    const long total = (long)N * H * W * C;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % C);
        long t = i / C;
        const int x = (int)(t % W);
        t /= W;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        dst[(((long)n * C + c) * H + y) * W + x] = (float)src[i] / 255.f;
    }
}

// ---- horizontal flip (MonoDataset.__getitem__'s do_flip: transpose(FLIP_LEFT_RIGHT) of the raw image BEFORE any resize).
// flip: one byte per item, nullptr = nobody.  A flagged item reads source column W-1-x wherever the plain kernel reads x, i.e. the
// kernel resamples the mirrored image; a mirrored row is the same contiguous span of memory, walked downwards.

// resample_h_kernel with per-item flags: row r belongs to item r / H
__global__ __launch_bounds__(TPB) void resample_h_flip_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int* __restrict__ bounds, const int* __restrict__ kk,
                                                              const uint8_t* __restrict__ flip, long rows, int H, int W, int OW, int C,
                                                              int ksize) {
    const long total = rows * OW * C;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % C);
        const long t = i / C;
        const int ox = (int)(t % OW);
        const long row = t / OW;
        const int xmin = bounds[2 * ox], xmax = bounds[2 * ox + 1];
        const int* k = kk + (long)ox * ksize;
        const bool fl = flip && flip[row / H];
        const uint8_t* sp = src + (row * W + (fl ? W - 1 - xmin : xmin)) * C + c;
        const long step = fl ? -(long)C : (long)C;
        int ss = 1 << (PBITS - 1);
        for (int x = 0; x < xmax; ++x) ss += (int)sp[x * step] * k[x];
        dst[i] = (uint8_t)clip8(ss);
    }
}

// (mirrored) HWC u8 -> CHW float / 255 and / or the (mirrored) HWC u8 image
__global__ __launch_bounds__(TPB) void to_tensor_flip_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst_f,
                                                             uint8_t* __restrict__ dst_u8, const uint8_t* __restrict__ flip, int N,
                                                             int H, int W, int C) {
    const long total = (long)N * H * W * C;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % C);
        long t = i / C;
        const int x = (int)(t % W);
        t /= W;                                             // t = n * H + y
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        const int sx = (flip && flip[n]) ? W - 1 - x : x;
        const uint8_t v = src[(t * W + sx) * C + c];
        if (dst_u8) dst_u8[i] = v;
        if (dst_f) dst_f[(((long)n * C + c) * H + y) * W + x] = (float)v / 255.f;
    }
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// per-image mean of the grayscale image (torchvision adjust_contrast): sums[n] = sum gray
__global__ __launch_bounds__(TPB) void gray_sum_kernel(const float* __restrict__ x, double* __restrict__ sums, int HW) {
    __shared__ double sm[4];
    const int n = blockIdx.y;
    const float* r = x + (size_t)n * 3 * HW;
    double s = 0.0;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) s += gray_of(r[i], r[HW + i], r[2 * HW + i]);
    s = jp_block_sum_d(s, sm);
    if (threadIdx.x == 0) atomicAdd(&sums[n], s);
}

// The four ColorJitter ops on one pixel, torchvision.transforms.functional (tensor path): _blend(img, other, f) =
// clamp(f*img + (1-f)*other).  ONE piece of code for color_jitter_kernel and the batched kernels below, so that the arithmetic
// (and the compiler's contraction of it) cannot differ between the per-op and the batched path.
__device__ __forceinline__ void cj_brightness(float& r, float& g, float& b, float f) {
    r = clamp01(r * f); g = clamp01(g * f); b = clamp01(b * f);
}
// mean: the gray mean of the whole image as it stands before this op
__device__ __forceinline__ void cj_contrast(float& r, float& g, float& b, float f, float mean) {
    const float m = mean * (1.f - f);
    r = clamp01(f * r + m); g = clamp01(f * g + m); b = clamp01(f * b + m);
}
__device__ __forceinline__ void cj_saturation(float& r, float& g, float& b, float f) {
    const float gr = gray_of(r, g, b) * (1.f - f);
    r = clamp01(f * r + gr); g = clamp01(f * g + gr); b = clamp01(f * b + gr);
}
__device__ __forceinline__ void cj_hue(float& r, float& g, float& b, float f) {
    // _rgb2hsv
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    const float hr = (maxc == r) ? (bc - gc) : 0.f;
    const float hg = ((maxc == g) && (maxc != r)) ? (2.f + rc - bc) : 0.f;
    const float hb = ((maxc != g) && (maxc != r)) ? (4.f + gc - rc) : 0.f;
    float h = fmodf(hr + hg + hb, 6.f) / 6.f + 1.f;          // torch.fmod keeps the dividend's sign
    h = fmodf(h, 1.f);
    h = fmodf(h + f, 1.f);
    if (h < 0.f) h += 1.f;                                    // python-style % on the shifted hue
    // _hsv2rgb
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fl = floorf(h6);
    const float ff = h6 - fl;
    const int i6 = ((int)fl) % 6;
    const float p_ = clamp01(v * (1.f - s)), q_ = clamp01(v * (1.f - s * ff)), t_ = clamp01(v * (1.f - s * (1.f - ff)));
    switch (i6) {
        case 0: r = v; g = t_; b = p_; break;
        case 1: r = q_; g = v; b = p_; break;
        case 2: r = p_; g = v; b = t_; break;
        case 3: r = p_; g = q_; b = v; break;
        case 4: r = t_; g = p_; b = v; break;
        default: r = v; g = p_; b = q_; break;
    }
}
// the pointwise ops by id (0 brightness, 2 saturation, 3 hue); contrast (1) needs the image's mean and is called by name
__device__ __forceinline__ void cj_pointwise(int op, float& r, float& g, float& b, float f) {
    if (op == 0) cj_brightness(r, g, b, f);
    else if (op == 2) cj_saturation(r, g, b, f);
    else if (op == 3) cj_hue(r, g, b, f);
}

// one ColorJitter op on (N,3,H,W) floats in place.  op: 0 brightness, 1 contrast (sums = per-image gray sums),
// 2 saturation, 3 hue
__global__ __launch_bounds__(TPB) void color_jitter_kernel(float* __restrict__ x, const double* __restrict__ sums, int N, int HW,
                                                           int op, float f) {
    const long total = (long)N * HW;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int n = (int)(i / HW), p = (int)(i - (long)n * HW);
        float* px = x + (size_t)n * 3 * HW + p;
        float r = px[0], g = px[HW], b = px[2 * HW];
        if (op == 1) cj_contrast(r, g, b, f, (float)(sums[n] / (double)HW));
        else cj_pointwise(op, r, g, b, f);
        px[0] = r; px[HW] = g; px[2 * HW] = b;
    }
}

// ---- batched ColorJitter: every image of the call has its own record in a device table
//   params[n] = JP_CJ_REC int32 words {n_ops (0..4), order[4] (op ids in the order they are applied), factor[4] (the bit
//   patterns of the floats; factor[j] belongs to order[j])}
// Two launches whatever N is.  Contrast needs the gray mean of the image as it stands after the ops before it: pass 1 recomputes those
// (pointwise) ops per pixel and leaves cj_partials(HW) partial gray sums per image in ws; pass 2 folds them in a fixed order (the same
// tree in every workgroup) and applies the whole chain.  No atomics: two runs give the same bits.
constexpr int JP_CJ_REC = 9;
constexpr int CJ_MAXPART = TPB;              // pass 2 folds one partial per thread
inline int cj_partials(int HW) { return std::min(jp_cdiv(HW, TPB), CJ_MAXPART); }

struct CjRec {
    int n_ops, cpos;                         // cpos: position of (the first) contrast in the order, -1 = none
    int op[4];
    float f[4];
};
__device__ __forceinline__ CjRec cj_load(const int* __restrict__ params, int n) {
    const int* p = params + (long)n * JP_CJ_REC;
    CjRec rc;
    rc.n_ops = min(max(p[0], 0), 4);
    rc.cpos = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rc.op[j] = p[1 + j];
        rc.f[j] = __int_as_float(p[5 + j]);
        if (rc.cpos < 0 && j < rc.n_ops && rc.op[j] == 1) rc.cpos = j;
    }
    return rc;
}

// pass 1, grid (cj_partials(HW), N): ws[n * parts + blockIdx.x] = this workgroup's share of sum gray(image n after ops [0, cpos))
__global__ __launch_bounds__(TPB) void cj_gray_partials_kernel(const float* __restrict__ x, const int* __restrict__ params,
                                                               double* __restrict__ ws, int HW) {
    __shared__ double sm[4];
    const int n = blockIdx.y;
    const CjRec rc = cj_load(params, n);
    if (rc.cpos < 0) return;                 // (uniform over the workgroup) no contrast: pass 2 does not read this image's partials
    const float* px = x + (size_t)n * 3 * HW;
    double s = 0.0;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < HW; i += (long)gridDim.x * TPB) {
        float r = px[i], g = px[HW + i], b = px[2L * HW + i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < rc.cpos) cj_pointwise(rc.op[j], r, g, b, rc.f[j]);
        s += gray_of(r, g, b);
    }
    s = jp_block_sum_d(s, sm);
    if (threadIdx.x == 0) ws[(long)n * gridDim.x + blockIdx.x] = s;
}

// pass 2, grid (<= 512, N): the whole chain of image n in place; an image with n_ops == 0 is not written
__global__ __launch_bounds__(TPB) void cj_apply_kernel(float* __restrict__ x, const int* __restrict__ params,
                                                       const double* __restrict__ ws, int HW, int parts) {
    __shared__ double sm[4];
    __shared__ float mean_s;
    const int n = blockIdx.y;
    const CjRec rc = cj_load(params, n);
    if (rc.n_ops == 0) return;
    float mean = 0.f;
    if (rc.cpos >= 0) {                      // every workgroup folds the image's partials in the same order
        const double v = jp_block_sum_d((int)threadIdx.x < parts ? ws[(long)n * parts + threadIdx.x] : 0.0, sm);
        if (threadIdx.x == 0) mean_s = (float)(v / (double)HW);
        __syncthreads();
        mean = mean_s;
    }
    float* px = x + (size_t)n * 3 * HW;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < HW; i += (long)gridDim.x * TPB) {
        float r = px[i], g = px[HW + i], b = px[2L * HW + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= rc.n_ops) break;
            if (rc.op[j] == 1) cj_contrast(r, g, b, rc.f[j], mean);
            else cj_pointwise(rc.op[j], r, g, b, rc.f[j]);
        }
        px[i] = r; px[HW + i] = g; px[2L * HW + i] = b;
    }
}

// BEV label: src (N, h, w, C) u8 (C = 1 or 3) -> dst (N, 1, S, S) float {0,1}: L = ITU-R 601 luma, NEAREST pick at
// floor((o + 0.5) * scale), then `>= thresh` (convert("1") without dithering: exact for the binary label images) or
// `== 255` (process_topview_both)
__global__ __launch_bounds__(TPB) void topview_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int N, int h, int w,
                                                      int C, int S, int exact255) {
    const long total = (long)N * S * S;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int ox = (int)(i % S);
        const long t = i / S;
        const int oy = (int)(t % S), n = (int)(t / S);
        const int sx = min(w - 1, (int)(((double)ox + 0.5) * (double)w / (double)S));
        const int sy = min(h - 1, (int)(((double)oy + 0.5) * (double)h / (double)S));
        const uint8_t* p = src + (((long)n * h + sy) * w + sx) * C;
        const int L = C == 1 ? (int)p[0] : (int)(((unsigned)p[0] * 19595u + (unsigned)p[1] * 38470u + (unsigned)p[2] * 7471u + 0x8000u) >> 16);
        dst[i] = exact255 ? (L == 255 ? 1.f : 0.f) : (L >= 128 ? 1.f : 0.f);
    }
}

// topview_kernel on the mirrored label of every flagged item: the NEAREST pick reads column w-1-sx
__global__ __launch_bounds__(TPB) void topview_flip_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst,
                                                           const uint8_t* __restrict__ flip, int N, int h, int w, int C, int S,
                                                           int exact255) {
    const long total = (long)N * S * S;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int ox = (int)(i % S);
        const long t = i / S;
        const int oy = (int)(t % S), n = (int)(t / S);
        int sx = min(w - 1, (int)(((double)ox + 0.5) * (double)w / (double)S));
        const int sy = min(h - 1, (int)(((double)oy + 0.5) * (double)h / (double)S));
        if (flip && flip[n]) sx = w - 1 - sx;
        const uint8_t* p = src + (((long)n * h + sy) * w + sx) * C;
        const int L = C == 1 ? (int)p[0] : (int)(((unsigned)p[0] * 19595u + (unsigned)p[1] * 38470u + (unsigned)p[2] * 7471u + 0x8000u) >> 16);
        dst[i] = exact255 ? (L == 255 ? 1.f : 0.f) : (L >= 128 ? 1.f : 0.f);
    }
}

inline int blocks_for(long n) { return (int)std::min<long>((n + TPB - 1) / TPB, 1 << 16); }
}  // namespace

#define JP_ST hipStream_t st = (hipStream_t)stream

// bounds: (out, 2) int32 {first tap, tap count}; kk: (out, ksize) int32 fixed-point coefficients (device copies of the
// host tables).  axis 0: horizontal, src (rows, W, C) -> dst (rows, OW, C)
extern "C" int jp_resample_h_u8(const uint8_t* src, uint8_t* dst, const int* bounds, const int* kk, long rows, int W, int OW,
                                int C, int ksize, void* stream) {
    JP_CHECK_ARG(src && dst && bounds && kk && rows > 0 && W > 0 && OW > 0 && C > 0 && ksize > 0, "resample_h_u8: bad args");
    JP_ST;
    hipLaunchKernelGGL(resample_h_kernel, dim3(blocks_for(rows * OW * C)), dim3(TPB), 0, st, src, dst, bounds, kk, rows, W, OW, C,
                       ksize);
    JP_LAUNCH_CHECK();
}

// vertical pass; writes uint8 HWC (out_u8) and / or float CHW / 255 (out_f = transforms.ToTensor of the resized image)
extern "C" int jp_resample_v_u8(const uint8_t* src, uint8_t* out_u8, float* out_f, const int* bounds, const int* kk, int N,
                                int H, int OH, int OW, int C, int ksize, void* stream) {
    JP_CHECK_ARG(src && (out_u8 || out_f) && bounds && kk && N > 0 && H > 0 && OH > 0 && OW > 0 && C > 0 && ksize > 0,
                 "resample_v_u8: bad args");
    JP_ST;
    hipLaunchKernelGGL(resample_v_kernel, dim3(blocks_for((long)N * OH * OW * C)), dim3(TPB), 0, st, src, out_u8, out_f, bounds,
                       kk, N, H, OH, OW, C, ksize);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_u8_to_tensor(const uint8_t* src, float* dst, int N, int H, int W, int C, void* stream) {
    JP_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0 && C > 0, "u8_to_tensor: bad args");
    JP_ST;
    hipLaunchKernelGGL(to_tensor_kernel, dim3(blocks_for((long)N * H * W * C)), dim3(TPB), 0, st, src, dst, N, H, W, C);
    JP_LAUNCH_CHECK();
}

// sums: N doubles of caller scratch (only read / written for op == 1)
extern "C" int jp_color_jitter_op(float* x, double* sums, int N, int HW, int op, float factor, void* stream) {
    JP_CHECK_ARG(x && N > 0 && HW > 0 && op >= 0 && op <= 3 && (op != 1 || sums), "color_jitter_op: bad args");
    JP_ST;
    if (op == 1) {
        JP_HIP(hipMemsetAsync(sums, 0, sizeof(double) * N, st));
        hipLaunchKernelGGL(gray_sum_kernel, dim3(std::min(jp_cdiv(HW, TPB), 256), N), dim3(TPB), 0, st, x, sums, HW);
    }
    hipLaunchKernelGGL(color_jitter_kernel, dim3(blocks_for((long)N * HW)), dim3(TPB), 0, st, x, sums, N, HW, op, factor);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_topview_u8(const uint8_t* src, float* dst, int N, int h, int w, int C, int S, int exact255, void* stream) {
    JP_CHECK_ARG(src && dst && N > 0 && h > 0 && w > 0 && (C == 1 || C == 3) && S > 0, "topview_u8: bad args");
    JP_ST;
    hipLaunchKernelGGL(topview_kernel, dim3(blocks_for((long)N * S * S)), dim3(TPB), 0, st, src, dst, N, h, w, C, S, exact255);
    JP_LAUNCH_CHECK();
}

// ---- horizontal flip + batched ColorJitter (the rest of MonoDataset.__getitem__'s training augmentation)
// flip: N bytes in device memory, one per item, non-zero = mirror that item left-right BEFORE the operation; NULL = no item.
// With flip == NULL or all-zero flags every entry point below writes what its plain counterpart writes, bit for bit.

// jp_resample_h_u8 over N items of H rows each: a flagged item's tap k of output column ox reads source column W-1-(xmin+k)
extern "C" int jp_resample_h_u8_flip(const uint8_t* src, uint8_t* dst, const int* bounds, const int* kk, const uint8_t* flip, int N,
                                     int H, int W, int OW, int C, int ksize, void* stream) {
    JP_CHECK_ARG(src && dst && bounds && kk && N > 0 && H > 0 && W > 0 && OW > 0 && C > 0 && ksize > 0,
                 "resample_h_u8_flip: bad args");
    JP_ST;
    const long rows = (long)N * H;
    hipLaunchKernelGGL(resample_h_flip_kernel, dim3(blocks_for(rows * OW * C)), dim3(TPB), 0, st, src, dst, bounds, kk, flip, rows, H, W,
                       OW, C, ksize);
    JP_LAUNCH_CHECK();
}

// no horizontal resize: (mirrored) src (N,H,W,C) -> dst_f (N,C,H,W) float / 255 and / or dst_u8 (N,H,W,C); either may be NULL, not
// both; dst_u8 must not be src (a mirror cannot be done in place)
extern "C" int jp_u8_to_tensor_flip(const uint8_t* src, float* dst_f, uint8_t* dst_u8, const uint8_t* flip, int N, int H, int W, int C,
                                    void* stream) {
    JP_CHECK_ARG(src && (dst_f || dst_u8) && dst_u8 != src && N > 0 && H > 0 && W > 0 && C > 0, "u8_to_tensor_flip: bad args");
    JP_ST;
    hipLaunchKernelGGL(to_tensor_flip_kernel, dim3(blocks_for((long)N * H * W * C)), dim3(TPB), 0, st, src, dst_f, dst_u8, flip, N, H, W,
                       C);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_topview_u8_flip(const uint8_t* src, float* dst, const uint8_t* flip, int N, int h, int w, int C, int S, int exact255,
                                  void* stream) {
    JP_CHECK_ARG(src && dst && N > 0 && h > 0 && w > 0 && (C == 1 || C == 3) && S > 0, "topview_u8_flip: bad args");
    JP_ST;
    hipLaunchKernelGGL(topview_flip_kernel, dim3(blocks_for((long)N * S * S)), dim3(TPB), 0, st, src, dst, flip, N, h, w, C, S, exact255);
    JP_LAUNCH_CHECK();
}

// doubles of caller scratch jp_color_jitter_batched needs for N images of HW pixels (need not be initialised)
extern "C" long jp_color_jitter_batched_ws_doubles(int N, int HW) {
    JP_CHECK_ARG(N > 0 && HW > 0, "color_jitter_batched_ws_doubles: N and HW must be positive");
    return (long)N * cj_partials(HW);
}

// ColorJitter on N images x (N,3,HW) in place, every image with its own record of the device table `params` (N x 9 int32 words:
// n_ops, order[4], factor[4] as float bits -- see JP_CJ_REC above); an image with n_ops == 0 is not written.  Two launches.
extern "C" int jp_color_jitter_batched(float* x, const int* params, double* ws, int N, int HW, void* stream) {
    JP_CHECK_ARG(x && params && ws && N > 0 && N <= 65535 && HW > 0, "color_jitter_batched: bad args");
    JP_ST;
    const int parts = cj_partials(HW);
    hipLaunchKernelGGL(cj_gray_partials_kernel, dim3(parts, N), dim3(TPB), 0, st, x, params, ws, HW);
    hipLaunchKernelGGL(cj_apply_kernel, dim3(std::min(jp_cdiv(HW, TPB), 512), N), dim3(TPB), 0, st, x, params, ws, HW, parts);
    JP_LAUNCH_CHECK();
}
