// Evaluation metrics of the reference as GPU reductions:
//   layout : confusion counts of argmax(topview logits) vs the BEV label  -> mean_IU / mean_precision
//            (mono/core/evaluation/pixel_error.py:59-118, eval_hooks.py:181-199)
//   depth  : Garg-crop + range mask, median scaling, clamp, the 7 error metrics
//            (pixel_error.py:27-40, eval_hooks.py:147-179)
// All host logic (class presence rules, averaging) stays in jperceiver_amd/core/evaluation.py.
#include "jp_common.h"
#include <algorithm>

namespace {
constexpr int TPB = 256;

// counts[b][2*p + t] += 1 for every pixel with prediction p = argmax(logits[b][:, pix]) (ties -> 0, like torch.argmax's
// first maximum) and label t = (gt != 0)
__global__ __launch_bounds__(TPB) void confusion2_kernel(const float* __restrict__ logits, const float* __restrict__ gt,
                                                         double* __restrict__ counts, int HW) {
    __shared__ double sm[4];
    const int b = blockIdx.y;
    const float* l0 = logits + (size_t)b * 2 * HW;
    const float* l1 = l0 + HW;
    const float* g = gt + (size_t)b * HW;
    int c[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
        const int p = l1[i] > l0[i] ? 1 : 0, t = g[i] != 0.f ? 1 : 0;
        c[2 * p + t] += 1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = jp_block_sum_d((double)c[k], sm);
        if (threadIdx.x == 0 && s != 0.0) atomicAdd(&counts[b * 4 + k], s);   // integer-valued doubles: order-independent
    }
}

// pred_depth = 1 / resized scaled disparity; valid = MIN < gt < MAX inside the Garg crop (eval_hooks.py:160-166)
__global__ __launch_bounds__(TPB) void depth_prepare_kernel(const float* __restrict__ disp_resized, const float* __restrict__ gt,
                                                            float* __restrict__ pred, uint8_t* __restrict__ valid, int H, int W,
                                                            int y0, int y1, int x0, int x1, float dmin, float dmax) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < H * W; i += gridDim.x * TPB) {
        const int y = i / W, x = i - y * W;
        const float g = gt[i];
        pred[i] = 1.f / disp_resized[i];
        valid[i] = (g > dmin && g < dmax && y >= y0 && y < y1 && x >= x0 && x < x1) ? 1 : 0;
    }
}

__device__ __forceinline__ unsigned ord_key(float f) {      // monotone float -> uint map
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_val(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// np.median over the valid elements: out[0] = count, out[1] = median (mean of the two central order statistics for an
// even count).  One workgroup, bit-wise bisection on the ordered key: 32 counting passes per order statistic.
__global__ __launch_bounds__(1024) void masked_median_kernel(const float* __restrict__ x, const uint8_t* __restrict__ valid,
                                                             int n, float* __restrict__ out) {
    __shared__ unsigned cnt;
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = threadIdx.x; i < n; i += 1024) mine += valid[i];
    atomicAdd(&total, mine);
    __syncthreads();
    const unsigned m = total;
    if (m == 0) {
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = __uint_as_float(0x7fc00000u); }
        return;
    }
    float res[2];
    const unsigned ks[2] = {(m - 1) / 2, m / 2};
    for (int which = 0; which < 2; ++which) {
        if (which == 1 && ks[1] == ks[0]) { res[1] = res[0]; break; }
        unsigned prefix = 0;                    // smallest key K with #(key <= K) >= k + 1, built from the top bit down
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = prefix | ((1u << bit) - 1u);      // largest key with this prefix and a 0 at `bit`
            __syncthreads();
            if (threadIdx.x == 0) cnt = 0;
            __syncthreads();
            unsigned c = 0;
            for (int i = threadIdx.x; i < n; i += 1024)
                if (valid[i] && ord_key(x[i]) <= cand) ++c;
            atomicAdd(&cnt, c);
            __syncthreads();
            if (cnt < ks[which] + 1) prefix |= 1u << bit;
        }
        res[which] = ord_val(prefix);
    }
    if (threadIdx.x == 0) { out[0] = (float)m; out[1] = 0.5f * (res[0] + res[1]); }
}

// sums[0..6] = a1, a2, a3 counts, sum (gt-p)^2, sum (log gt - log p)^2, sum |gt-p|/gt, sum (gt-p)^2/gt; sums[7] = count
// with p = clamp(pred * ratio, dmin, dmax), ratio = med[1] (gt) / med[3] (pred) unless fixed_scale > 0
__global__ __launch_bounds__(TPB) void depth_errors_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                           const uint8_t* __restrict__ valid, int n,
                                                           const float* __restrict__ med_gt, const float* __restrict__ med_pred,
                                                           float fixed_scale, float dmin, float dmax, double* __restrict__ sums) {
    __shared__ double sm[4];
    const float ratio = fixed_scale > 0.f ? fixed_scale : med_gt[1] / med_pred[1];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        if (!valid[i]) continue;
        const float g = gt[i];
        const float p = fminf(fmaxf(pred[i] * ratio, dmin), dmax);
        const float th = fmaxf(g / p, p / g), d = g - p, lg = logf(g) - logf(p);
        acc[0] += th < 1.25f;
        acc[1] += th < 1.25f * 1.25f;
        acc[2] += th < 1.25f * 1.25f * 1.25f;
        acc[3] += (double)d * d;
        acc[4] += (double)lg * lg;
        acc[5] += fabsf(d) / g;
        acc[6] += (double)d * d / g;
        acc[7] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double s = jp_block_sum_d(acc[k], sm);
        if (threadIdx.x == 0) atomicAdd(&sums[k], s);
    }
}
// ------------------------------------------------------------------ batched depth scorer (jp_depth_eval_batch)
// The chain of core/evaluation.py::eval_depth for B images in four launches and without atomics on floating-point data: two runs
// give the same bits.  gridDim.y = item everywhere.
constexpr int DEB_MAX_BLOCKS = 128;                 // error partials per item: a fixed grid makes the fold order a function of H W alone

// the sampling rule of jp_bilinear_fwd (pointwise.hip:bil_src)
__device__ __forceinline__ void deb_src(int o, float scale, int in, int& i0, int& i1, float& w1) {
    float src = ((float)o + 0.5f) * scale - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    w1 = src - (float)i0;
}

// jp_affine -> jp_bilinear_fwd -> depth_prepare_kernel in one pass: the same float32 operations per pixel, in the same expressions
// (the affine map of the four taps, the bilinear blend, 1 / x), so pred and valid hold the bits the three launches leave
__global__ __launch_bounds__(TPB) void deb_prepare_kernel(const float* __restrict__ disp, const float* __restrict__ gt,
                                                          float* __restrict__ pred, uint8_t* __restrict__ valid, int h, int w, int H,
                                                          int W, float sy, float sx, float scale, float shift, int y0, int y1, int x0,
                                                          int x1, float dmin, float dmax) {
    const int b = blockIdx.y;
    const float* dp = disp + (size_t)b * h * w;
    const float* g = gt + (size_t)b * H * W;
    float* pr = pred + (size_t)b * H * W;
    uint8_t* va = valid + (size_t)b * H * W;
    for (int i = blockIdx.x * TPB + threadIdx.x; i < H * W; i += gridDim.x * TPB) {
        const int y = i / W, x = i - y * W;
        int ya, yb, xa, xb;
        float wy, wx;
        deb_src(y, sy, h, ya, yb, wy);
        deb_src(x, sx, w, xa, xb, wx);
        const float a = dp[ya * w + xa] * scale + shift, bq = dp[ya * w + xb] * scale + shift;
        const float c = dp[yb * w + xa] * scale + shift, d = dp[yb * w + xb] * scale + shift;
        const float s = (1.f - wy) * ((1.f - wx) * a + wx * bq) + wy * ((1.f - wx) * c + wx * d);
        const float gv = g[i];
        pr[i] = 1.f / s;
        va[i] = (gv > dmin && gv < dmax && y >= y0 && y < y1 && x >= x0 && x < x1) ? 1 : 0;
    }
}

// h[digit] += 1 for the lanes with m set; must be reached by all 64 lanes.  Depth data puts whole waves into one bin in the leading
// pass (same sign and exponent), which per-lane LDS atomics serialise: a wave that agrees on the bin adds its count once.
__device__ __forceinline__ void deb_hist_add(unsigned* h, unsigned digit, bool m) {
    const unsigned long long bal = __ballot(m);
    if (bal == 0) return;
    const int first = __ffsll((long long)bal) - 1;
    const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
    if (__ballot(m && digit != d0) == 0) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[d0], (unsigned)__popcll(bal));
    } else if (m) {
        atomicAdd(&h[digit], 1u);
    }
}

// masked_median_kernel's result ({count, np.median}) by exact radix selection on the same ordered key: 4 counting passes of 8 key bits
// for the lower central order statistic, one more pass for the upper one (the same value when enough elements tie with the lower one,
// the smallest larger key otherwise) instead of 32 passes for each.  blockIdx.x: 0 = ground truth, 1 = prediction; blockIdx.y = item:
// one workgroup each.  Integer counts only: the result does not depend on the order of the LDS atomics.
__global__ __launch_bounds__(1024) void deb_median_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                          const uint8_t* __restrict__ valid, int n, float* __restrict__ med) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_k, s_total, s_cnt, s_min;
    const int b = blockIdx.y;
    const float* x = (blockIdx.x == 0 ? gt : pred) + (size_t)b * n;
    const uint8_t* va = valid + (size_t)b * n;
    float* out = med + (size_t)b * 4 + 2 * blockIdx.x;
    unsigned prefix = 0, k = 0, total = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int base = 0; base < n; base += 1024) {                 // wave-uniform trip count
            const int i = base + threadIdx.x;
            bool m = i < n && va[i];
            unsigned key = 0;
            if (m) {
                key = ord_key(x[i]);
                m = pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8));
            }
            deb_hist_add(hist, (key >> shift) & 255u, m);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (pass == 0) {
                unsigned t = 0;
                for (int d = 0; d < 256; ++d) t += hist[d];
                s_total = t;
                k = t ? (t - 1) / 2 : 0;
            }
            unsigned cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                if (cum + hist[d] > k) break;
                cum += hist[d];
            }
            s_prefix = prefix | ((unsigned)d << shift);
            s_k = k - cum;
            s_cnt = 0;
            s_min = 0xffffffffu;
        }
        __syncthreads();
        prefix = s_prefix, k = s_k, total = s_total;
        if (total == 0) {
            if (threadIdx.x == 0) { out[0] = 0.f; out[1] = __uint_as_float(0x7fc00000u); }
            return;
        }
    }
    const float lo = ord_val(prefix);
    float hi = lo;
    if (total / 2 != (total - 1) / 2) {
        unsigned c = 0, mn = 0xffffffffu;
        for (int i = threadIdx.x; i < n; i += 1024) {
            if (!va[i]) continue;
            const unsigned key = ord_key(x[i]);
            if (key <= prefix) ++c;
            else mn = min(mn, key);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += (unsigned)__shfl_xor((int)c, o, 64);
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o, 64));
        }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&s_cnt, c); atomicMin(&s_min, mn); }
        __syncthreads();
        hi = s_cnt >= total / 2 + 1 ? lo : ord_val(s_min);
    }
    if (threadIdx.x == 0) { out[0] = (float)total; out[1] = 0.5f * (lo + hi); }
}

// depth_errors_kernel's eight sums of one item as per-workgroup partials: part[b][blockIdx.x][0..7]
__global__ __launch_bounds__(TPB) void deb_errors_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         const uint8_t* __restrict__ valid, int n, const float* __restrict__ med,
                                                         float fixed_scale, float dmin, float dmax, double* __restrict__ part) {
    __shared__ double sm[4];
    const int b = blockIdx.y;
    const float* g_ = gt + (size_t)b * n;
    const float* p_ = pred + (size_t)b * n;
    const uint8_t* va = valid + (size_t)b * n;
    const float ratio = fixed_scale > 0.f ? fixed_scale : med[b * 4 + 1] / med[b * 4 + 3];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        if (!va[i]) continue;
        const float g = g_[i];
        const float p = fminf(fmaxf(p_[i] * ratio, dmin), dmax);
        const float th = fmaxf(g / p, p / g), d = g - p, lg = logf(g) - logf(p);
        acc[0] += th < 1.25f;
        acc[1] += th < 1.25f * 1.25f;
        acc[2] += th < 1.25f * 1.25f * 1.25f;
        acc[3] += (double)d * d;
        acc[4] += (double)lg * lg;
        acc[5] += fabsf(d) / g;
        acc[6] += (double)d * d / g;
        acc[7] += 1.0;
    }
    double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double s = jp_block_sum_d(acc[k], sm);
        if (threadIdx.x == 0) o[k] = s;
    }
}

// sums[b][k] = part[b][0][k] + part[b][1][k] + ... in that order
__global__ __launch_bounds__(64) void deb_fold_kernel(const double* __restrict__ part, int nblk, double* __restrict__ sums) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 8) return;
    double s = 0.0;
    for (int j = 0; j < nblk; ++j) s += part[((size_t)b * nblk + j) * 8 + k];
    sums[b * 8 + k] = s;
}

inline int deb_blocks(long hw) { return std::min(jp_cdiv(hw, TPB), DEB_MAX_BLOCKS); }
inline long deb_align(long v) { return (v + 255) / 256 * 256; }
}  // namespace

#define JP_ST hipStream_t st = (hipStream_t)stream

extern "C" int jp_confusion2(const float* logits, const float* gt, double* counts, int B, int HW, void* stream) {
    JP_CHECK_ARG(logits && gt && counts && B > 0 && HW > 0, "confusion2: bad args");
    JP_ST;
    JP_HIP(hipMemsetAsync(counts, 0, sizeof(double) * 4 * B, st));
    hipLaunchKernelGGL(confusion2_kernel, dim3(std::min(jp_cdiv(HW, TPB), 64), B), dim3(TPB), 0, st, logits, gt, counts, HW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_depth_eval_prepare(const float* disp_resized, const float* gt, float* pred, uint8_t* valid, int H, int W,
                                     int y0, int y1, int x0, int x1, float dmin, float dmax, void* stream) {
    JP_CHECK_ARG(disp_resized && gt && pred && valid && H > 0 && W > 0, "depth_eval_prepare: bad args");
    JP_ST;
    hipLaunchKernelGGL(depth_prepare_kernel, dim3(std::min(jp_cdiv(H * W, TPB), 2048)), dim3(TPB), 0, st, disp_resized, gt, pred,
                       valid, H, W, y0, y1, x0, x1, dmin, dmax);
    JP_LAUNCH_CHECK();
}

// out: 2 floats {count, median}
extern "C" int jp_masked_median(const float* x, const uint8_t* valid, int n, float* out, void* stream) {
    JP_CHECK_ARG(x && valid && out && n > 0, "masked_median: bad args");
    JP_ST;
    hipLaunchKernelGGL(masked_median_kernel, dim3(1), dim3(1024), 0, st, x, valid, n, out);
    JP_LAUNCH_CHECK();
}

// sums: 8 doubles (zeroed here)
extern "C" int jp_depth_errors(const float* gt, const float* pred, const uint8_t* valid, int n, const float* med_gt,
                               const float* med_pred, float fixed_scale, float dmin, float dmax, double* sums, void* stream) {
    JP_CHECK_ARG(gt && pred && valid && sums && n > 0 && (fixed_scale > 0.f || (med_gt && med_pred)), "depth_errors: bad args");
    JP_ST;
    JP_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 8, st));
    hipLaunchKernelGGL(depth_errors_kernel, dim3(std::min(jp_cdiv(n, TPB), 1024)), dim3(TPB), 0, st, gt, pred, valid, n, med_gt,
                       med_pred, fixed_scale, dmin, dmax, sums);
    JP_LAUNCH_CHECK();
}

// Workspace of jp_depth_eval_batch: pred (B, H, W) floats, valid (B, H, W) bytes, the error partials (B, blocks, 8) doubles
extern "C" long jp_depth_eval_batch_ws_bytes(int B, int H, int W) {
    if (!(B > 0 && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL)) {
        jp_set_last_error("depth_eval_batch_ws_bytes: B, H, W must be positive and H * W fit an int");
        return JP_EBADARG;
    }
    const long hw = (long)H * W;
    return deb_align(4 * B * hw) + deb_align(B * hw) + (long)B * deb_blocks(hw) * 8 * (long)sizeof(double);
}

// eval_depth's chain for B images: disp (B,1,h,w) network output, gt (B,H,W); scaled disparity 1/max_depth + (1/min_depth -
// 1/max_depth) disp (the two constants are formed in double and rounded to float once, as the Python chain does) -> half-pixel
// bilinear resize -> 1/x, valid = mask_min < gt < mask_max inside rows y0..y1-1, columns x0..x1-1 -> both masked medians ->
// clamp(pred * ratio, mask_min, mask_max) with ratio = median gt / median pred (fixed_scale > 0: that instead) -> sums (B,8) as
// jp_depth_errors defines them, med (B,4) = {n, median gt, n, median pred}.  sums, med and ws need not be initialised.
extern "C" int jp_depth_eval_batch(const float* disp, const float* gt, int B, int h, int w, int H, int W, int y0, int y1, int x0,
                                   int x1, float mask_min, float mask_max, double min_depth, double max_depth, float fixed_scale,
                                   double* sums, float* med, void* ws, void* stream) {
    JP_CHECK_ARG(disp && gt && sums && med && ws, "depth_eval_batch: null disp, gt, sums, med or ws");
    JP_CHECK_ARG(B > 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL && (long)h * w <= 0x7fffffffL,
                 "depth_eval_batch: 1 <= B <= 65535 and positive sizes whose products fit an int");
    JP_CHECK_ARG(min_depth > 0.0 && max_depth > 0.0, "depth_eval_batch: min_depth and max_depth must be positive");
    JP_ST;
    const long hw = (long)H * W;
    const int nblk = deb_blocks(hw);
    float* pred = (float*)ws;
    uint8_t* valid = (uint8_t*)ws + deb_align(4 * B * hw);
    double* part = (double*)((uint8_t*)ws + deb_align(4 * B * hw) + deb_align(B * hw));
    const float scale = (float)(1.0 / min_depth - 1.0 / max_depth), shift = (float)(1.0 / max_depth);
    hipLaunchKernelGGL(deb_prepare_kernel, dim3(std::min(jp_cdiv(hw, TPB), 2048), B), dim3(TPB), 0, st, disp, gt, pred, valid, h, w, H,
                       W, (float)h / (float)H, (float)w / (float)W, scale, shift, y0, y1, x0, x1, mask_min, mask_max);
    hipLaunchKernelGGL(deb_median_kernel, dim3(2, B), dim3(1024), 0, st, gt, (const float*)pred, (const uint8_t*)valid, (int)hw, med);
    hipLaunchKernelGGL(deb_errors_kernel, dim3(nblk, B), dim3(TPB), 0, st, gt, (const float*)pred, (const uint8_t*)valid, (int)hw,
                       (const float*)med, fixed_scale, mask_min, mask_max, part);
    hipLaunchKernelGGL(deb_fold_kernel, dim3(B), dim3(64), 0, st, (const double*)part, nblk, sums);
    JP_LAUNCH_CHECK();
}
