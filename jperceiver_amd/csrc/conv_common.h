// What conv_fwd.hip, conv_dgrad.hip and conv_wgrad.hip share: the source descriptor, the pixel decode and generic gather, the scratch
// epilogue of the split-K launches, the launch helpers of the generic engine, and the prototypes of conv_small.hip / conv_c16.hip.
// In an anonymous namespace or inline, as in the single unit these were cut from; not part of the ABI.  conv_fwd.hip's head has the
// GEMM shapes; what only forward and dgrad share (the patch-kernel launch layer) is in conv_launch.h.
#pragma once
#include "igemm.h"
#include "scale.h"
#include <algorithm>
#include <cstdlib>

namespace {

struct Src3 {  // input as up to 3 channel segments, each optionally stored at half resolution
    const float *p0, *p1, *p2;
    int e0, e1, e2;     // cumulative channel ends
    int s0, s1, s2;     // 1 = segment stored at half resolution (fused nearest 2x upsample)
    int H, W;           // logical spatial size seen by the convolution
    __device__ __forceinline__ float at(int img, int ci, int iy, int ix) const {
        // scalar selects only: runtime-indexed member arrays would be spilled to scratch
        const bool a = ci < e0, b = ci < e1;
        const float* p = a ? p0 : (b ? p1 : p2);
        const int c0 = a ? 0 : (b ? e0 : e1);
        const int Cs = a ? e0 : (b ? e1 - e0 : e2 - e1);
        const int sh = a ? s0 : (b ? s1 : s2);
        const int h = H >> sh, w = W >> sh;
        return p[((size_t)(img * Cs + (ci - c0)) * h + (iy >> sh)) * w + (ix >> sh)];
    }
};

struct PixSt {  // decoded output pixel of a conv
    int img, iy0, ix0, valid;
};

__device__ __forceinline__ PixSt conv_pix(int p, int Npix, int OH, int OW, int stride, int pad) {
    PixSt st;
    st.valid = p < Npix;
    int ohw = OH * OW;
    st.img = p / ohw;
    int pix = p - st.img * ohw;
    int oy = pix / OW, ox = pix - oy * OW;
    st.iy0 = oy * stride - pad;
    st.ix0 = ox * stride - pad;
    return st;
}

template <int KH>
__device__ __forceinline__ float conv_gather(const Src3& src, const PixSt& st, int k, int reflect) {
    int ci = k / (KH * KH);
    int tap = k - ci * (KH * KH);
    int dy = tap / KH, dx = tap - dy * KH;
    int iy = st.iy0 + dy, ix = st.ix0 + dx;
    if (reflect) {
        iy = jp_reflect(iy, src.H);
        ix = jp_reflect(ix, src.W);
    } else if ((unsigned)iy >= (unsigned)src.H || (unsigned)ix >= (unsigned)src.W) {
        return 0.f;
    }
    return src.at(st.img, ci, iy, ix);
}

struct WgradEpiWS {  // split-K partial tiles as plain stores into caller scratch ws[split][m][n]; wgrad_reduce sums them
    typedef int St;
    float* ws;
    int M, Np;
    __device__ __forceinline__ St col(int n) const { return n; }
    static constexpr bool WANTS_SLICE = true;
    __device__ __forceinline__ void put(St n, int m, float v, int slice) const { ws[((size_t)slice * M + m) * Np + n] = v; }
};

constexpr int KC = 32;

// IL: gather interleaved with the MFMAs (measured +6 % on wgrad, -6 % on fwd/dgrad -> wgrad only)
template <bool IL, int WM, int WN, class A, class B, class E>
void launch(A a, B b, E e, int M, int N, int K, int splits, int kps, hipStream_t st) {
    dim3 grid(jp_cdiv(N, 64 * WN), jp_cdiv(M, 64 * WM), splits);
    jp_prof_before(__PRETTY_FUNCTION__, 2.0 * M * (double)N * K, st);
    hipLaunchKernelGGL((jp_igemm_kernel<WM, WN, KC, A, B, E, false, IL>), grid, dim3(64 * WM * WN), 0, st, a, b, e, M, N, K, kps);
    jp_prof_after(st);
}

template <bool IL = false, class A, class B, class E>
void launch_auto(A a, B b, E e, int M, int N, int K, int splits, int kps, hipStream_t st) {
    if (M <= 64) launch<IL, 1, 4>(a, b, e, M, N, K, splits, kps, st);
    else if (N <= 64) launch<IL, 4, 1>(a, b, e, M, N, K, splits, kps, st);
    else launch<IL, 2, 2>(a, b, e, M, N, K, splits, kps, st);
}

Src3 make_src(const float* x0, int c0, int up0, const float* x1, int c1, int up1, const float* x2, int c2,
              int up2, int H, int W) {
    Src3 s;
    s.p0 = x0; s.p1 = x1 ? x1 : x0; s.p2 = x2 ? x2 : x0;
    s.e0 = c0; s.e1 = c0 + c1; s.e2 = c0 + c1 + c2;
    s.s0 = up0; s.s1 = up1; s.s2 = up2;
    s.H = H; s.W = W;
    return s;
}

inline int pad32(int c) { return (c + 31) / 32 * 32; }

}  // namespace

// conv_small.hip: direct kernels for <= 4 output channels (disparity / BEV logits heads)
int jp_conv_small_fwd(const float* x0, int c0, int up0, const float* x1, int c1, int up1, const float* x2, int c2, int up2,
                      const float* w, const float* bias, float* y, int N, int H, int W, int Cout, int act, int reflect,
                      hipStream_t st, int accumulate = 0);
long jp_conv_small_wgrad_ws_floats(int N, int Cin, int H, int W, int Cout, int single_full_res);
int jp_conv_small_wgrad(const float* x0, int c0, int up0, const float* x1, int c1, int up1, const float* x2, int c2, int up2,
                        const float* dy, float* dw, int N, int H, int W, int Cout, int reflect, hipStream_t st, float* ws,
                        long ws_floats);
// conv_c16.hip: direct kernels for the 16 / 32-channel 3x3 layers of the BEV decoder
bool jp_c16_ok(int Cin, int Cout, int KH, int stride, int pad, int pad_mode, int H, int W);
int jp_c16_fwd(const float* x, int up, const float* w, const float* bias, float* y, int N, int Cin, int Cout, int H, int W, int act,
               hipStream_t st);
int jp_c16_dgrad(const float* dy, const float* w, float* dx, int up, int N, int Cin, int Cout, int H, int W, int accumulate,
                 hipStream_t st);
int jp_c16_wgrad(const float* x, int up, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W, hipStream_t st,
                 float* ws, long ws_floats);
long jp_c16_wgrad_ws_floats(int N, int Cin, int Cout, int H, int W);
int jp_up_head_fwd(const float* x, const float* w, const float* bias, float* y, int N, int C, int h, int wd, int act,
                   hipStream_t st);
int jp_up_head_dgrad(const float* dy, const float* w, float* dx, int N, int C, int h, int wd, int accumulate, hipStream_t st);
long jp_up_head_wgrad_ws_floats(int N, int C, int h, int wd);
int jp_up_head_wgrad(const float* x, const float* dy, float* dw, int N, int C, int h, int wd, hipStream_t st, float* ws,
                     long ws_floats);
// one-channel head on a single nearest-2x-upsampled source (the disparity heads): upsample-aware direct kernels
static inline bool up_head(int c0, int up0, int c1, int c2, int Cout, int KH, int stride, int pad, int pad_mode, int H, int W) {
    return Cout == 1 && c1 == 0 && c2 == 0 && up0 && c0 >= 8 && c0 <= 768 && KH == 3 && stride == 1 && pad == 1 &&
           pad_mode == JP_PAD_REFLECT && H % 2 == 0 && W % 2 == 0 && H >= 4 && W >= 4;
}
static inline bool small_head(int Cin, int Cout, int KH, int stride, int pad) {
    return Cout <= 4 && KH == 3 && stride == 1 && pad == 1 && (long)Cout * Cin * 9 * 4 <= 48 * 1024;
}

#define JP_KH_SWITCH(KHV, ...)                                  \
    switch (KHV) {                                              \
        case 1: { constexpr int KH_ = 1; __VA_ARGS__; } break;  \
        case 3: { constexpr int KH_ = 3; __VA_ARGS__; } break;  \
        case 7: { constexpr int KH_ = 7; __VA_ARGS__; } break;  \
        default: jp_set_last_error("conv: kernel size must be 1, 3 or 7"); return JP_EBADARG; \
    }
