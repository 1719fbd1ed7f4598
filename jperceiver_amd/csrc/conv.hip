// conv2d forward / dgrad / wgrad for the JPerceiver train step as instances of the fp32-MFMA
// implicit-GEMM engine (igemm.h).  Forward and dgrad are in this unit, wgrad is in
// conv_wgrad.hip, what both use is in conv_common.h.  Replaces every nn.Conv2d /
// ReflectionPad2d+Conv2d call site of the reference hot path (resnet.py:6-13,91; layers.py:147-167; depth_decoder.py:15-39;
// pose_decoder.py:9-12; layout_model.py:31-47,138-153; CrossViewTransformer.py:30-42).
//
// Layout: activations NCHW fp32, weights [Cout][Cin][KH][KW] fp32 (the reference's state-dict
// layout, so checkpoints stay interchangeable).
//   forward : M = Cout,  N = batch*OH*OW pixels,  K = taps*Cin    (B gathered with zero/reflect
//             padding, stride, and optional fused nearest-2x-upsample + channel-concat sources)
//   dgrad   : M = Cin,   N = batch*H*W  pixels,   K = taps*Cout   (B gathers dY; the adjoint of
//             reflection padding is folded into the gather, no workspace)
//   wgrad   : M = Cout,  N = taps*Cin,            K = batch*OH*OW (split-K; partial tiles reduced
//             through caller scratch, or fp32 atomics without it)
//
// Loader families (DESIGN.md §4.1 has the measurements behind each):
//   "T"  tap-major fast path: K ordered (channel chunk of 32, tap, channel); tap decode, bounds / reflection and source
//        selection once per chunk; scalar-base addressing (wave-uniform 64-bit base + per-lane 32-bit offset); weights
//        re-packed per launch to [tap][row][channel_pad32] (L2-resident, conv_pack.hip) so the A loads are coalesced.
//   "R3" row-tile kernel for 3x3 stride-1 layers whose pixel tile is one image-row segment: the three dx taps share one
//        staged row segment (forward and dgrad main pass).
//   "P"  parity-class kernels for inputs read through the fused nearest-2x upsample (iconv layers, disparity heads):
//        4 pre-summed weight slots per output parity instead of 9 taps, in forward, dgrad and wgrad.
//   "S2" parity-class dgrad of the 3x3 stride-2 convs; "C" whole-tap K chunks for the 3/6-channel stems.
//   "G"  generic (channel-major K, per-element decode): whatever the fast paths do not cover.
#include "conv_common.h"
#include "conv_pack.h"
#include "igemm_p9.h"
#include "igemm_p9s.h"
#include "conv_p9sm.h"
#include "igemm_p9us2.h"
#if JP_NS == 3
#include "igemm_p1l.h"      // the persistent 1x1 kernel exists in the six-product build only (opt-in there, JP_P1L=1)
#endif
#include "scale.h"
constexpr double JP_NPROD = JP_NS == 2 ? 3.0 : 6.0;     // matrix-pipe products per fp32 product of the P9S-family kernels
#include "igemm_p9sd.h"
#include "igemm_p9s2d.h"
#include "igemm_p9s2f.h"
#include "igemm_p7s.h"
#include "igemm_p9u.h"
#include <algorithm>
#include <cstdlib>

namespace {

// Masked-out gathers read this word instead of branching around the load: the gather stays a straight run of
// unconditional global loads (no exec-mask save/restore per element).
__device__ float jp_zero_word[4] = {0.f, 0.f, 0.f, 0.f};

// =============================================================== generic (channel-major K) loaders
struct FwdA {  // A[m=co][k] = W[co*K + k]
    static constexpr bool ALONG_K = true;
    typedef int St;
    const float* w;
    int M, K;
    __device__ __forceinline__ void init(St&, int, int) const {}
    __device__ __forceinline__ void fix(St& st, int k) const { st = k; }
    __device__ __forceinline__ float get(St k, int m, int) const { return (m < M && k < K) ? w[(size_t)m * K + k] : 0.f; }
};

struct PixKSt {
    PixSt px;
    int kc;
};

template <int KH>
struct FwdB {  // B[k=(ci,dy,dx)][n=pixel]
    static constexpr bool ALONG_K = false;
    typedef PixKSt St;
    Src3 src;
    int K, Npix, OH, OW, stride, pad, reflect;
    __device__ __forceinline__ void init(St& st, int p) const { st = St{conv_pix(p, Npix, OH, OW, stride, pad), 0}; }
    __device__ __forceinline__ void chunk(St& st, int kc) const { st.kc = kc; }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const int k = st.kc + kl;
        if (!st.px.valid || k >= K) return 0.f;
        return conv_gather<KH>(src, st.px, k, reflect);
    }
};

struct FwdEpi {  // y[img][co][pix] = act(acc + bias[co])
    typedef size_t St;
    float* y;
    const float* bias;
    int Cout, OHW, act;
    unsigned* amax = nullptr;           // != nullptr: the patch kernels report max |y| here (the entry point's amax_y)
    float* stats = nullptr;             // != nullptr: BatchNorm statistics partials of y (the entry point's bn_stats), igemm_p9s.h epilogue
    __device__ __forceinline__ St col(int p) const {
        int img = p / OHW;
        return (size_t)img * Cout * OHW + (p - img * OHW);
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        if (bias) v += bias[m];
        y[base + (size_t)m * OHW] = jp_act(v, act);
    }
    __device__ __forceinline__ float put_get(St base, int m, float v) const {       // put, returning the stored value
        if (bias) v += bias[m];
        const float r = jp_act(v, act);
        y[base + (size_t)m * OHW] = r;
        return r;
    }
    __device__ __forceinline__ float put4_get(St base, int m, float4 v) const {     // put4, returning the largest stored magnitude
        const float b = bias ? bias[m] : 0.f;
        const float4 r = make_float4(jp_act(v.x + b, act), jp_act(v.y + b, act), jp_act(v.z + b, act), jp_act(v.w + b, act));
        *reinterpret_cast<float4*>(y + base + (size_t)m * OHW) = r;
        return fmaxf(fmaxf(jp_fmag(r.x), jp_fmag(r.y)), fmaxf(jp_fmag(r.z), jp_fmag(r.w)));
    }
    // four consecutive pixels of channel m (16-byte aligned: the patch kernels' tiles start at multiples of 32 pixels)
    __device__ __forceinline__ void put4(St base, int m, float4 v) const {
        const float b = bias ? bias[m] : 0.f;
        *reinterpret_cast<float4*>(y + base + (size_t)m * OHW) =
            make_float4(jp_act(v.x + b, act), jp_act(v.y + b, act), jp_act(v.z + b, act), jp_act(v.w + b, act));
    }
};

struct AtomicEpi {  // out[img][m][pix] += acc : split-K forward / dgrad on grids too small to fill the chip
    typedef size_t St;
    float* out;
    int C, HW;
    __device__ __forceinline__ St col(int p) const {
        int img = p / HW;
        return (size_t)img * C * HW + (p - img * HW);
    }
    __device__ __forceinline__ void put(St base, int m, float v) const { atomicAdd(out + base + (size_t)m * HW, v); }
};

__global__ void bias_act_nchw_kernel(float* __restrict__ y, const float* __restrict__ bias, long total, int C, int HW,
                                     int act) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)((i / HW) % C);
        y[i] = jp_act(y[i] + (bias ? bias[c] : 0.f), act);
    }
}

// deterministic small-grid split-K: y[img][m][pix] = act(bias[m] + sum_s part[s][m][n]) in a fixed order
__global__ void slice_reduce_nchw_kernel(const float* __restrict__ part, float* __restrict__ y,
                                         const float* __restrict__ bias, int M, int Npix, int HW, int splits, int act,
                                         int accumulate) {
    const long total = (long)M * Npix;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / Npix), n = (int)(i - (long)m * Npix);
        float s = bias ? bias[m] : 0.f;
        for (int k = 0; k < splits; ++k) s += part[(size_t)k * total + i];
        const int img = n / HW;
        float* q = y + ((size_t)img * M + m) * HW + (n - img * HW);
        *q = accumulate ? *q + jp_act(s, act) : jp_act(s, act);
    }
}
void slice_reduce_nchw(const float* part, float* y, const float* bias, int M, int Npix, int HW, int splits, int act, int accumulate,
                       hipStream_t st) {
    const long total = (long)M * Npix;
    hipLaunchKernelGGL(slice_reduce_nchw_kernel, dim3((int)std::min<long>((total + 255) / 256, 2048)), dim3(256), 0, st, part, y, bias, M,
                       Npix, HW, splits, act, accumulate);
}

struct MKSt {
    int m, kc;
};

template <int KH>
struct DgradA {  // A[m=ci][k=(co,dy,dx)] = W[co][ci][dy][dx]
    static constexpr bool ALONG_K = false;
    typedef MKSt St;
    const float* w;
    int Cin, K;
    __device__ __forceinline__ void init(St& st, int m) const { st = St{m, 0}; }
    __device__ __forceinline__ void chunk(St& st, int kc) const { st.kc = kc; }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const int k = st.kc + kl;
        if (st.m >= Cin || k >= K) return 0.f;
        int co = k / (KH * KH);
        int tap = k - co * (KH * KH);
        return w[((size_t)co * Cin + st.m) * (KH * KH) + tap];
    }
};

struct InPixSt {
    int img, y, x, valid;
};

// offsets (within one dY channel plane) of the dY entries that touched input pixel (y,x) through tap (ty,tx):
// zero padding: at most one; ReflectionPad2d(1) + 3x3 stride 1: padded row py in [0,H+1] maps to input row
// reflect(py-1); input row y is hit by py=y+1 and additionally by py=0 when y==1 and py=H+1 when y==H-2;
// the dY row is py - ty and must lie in [0,H) -> at most 2 rows x 2 cols.
struct DyOffs {
    int o0, o1, o2, o3;
};
__device__ __forceinline__ DyOffs dy_offsets(int y, int x, int ty, int tx, int H, int W, int OH, int OW, int stride,
                                             int pad, int reflect) {
    DyOffs d{-1, -1, -1, -1};
    if (!reflect) {
        int ny = y + pad - ty, nx = x + pad - tx;
        if (ny < 0 || nx < 0) return d;
        int oy = ny / stride, ox = nx / stride;
        if (oy * stride != ny || ox * stride != nx || oy >= OH || ox >= OW) return d;
        d.o0 = oy * OW + ox;
        return d;
    }
    int r0 = y + 1 - ty, r1 = -1, c0 = x + 1 - tx, c1 = -1;
    if (r0 < 0 || r0 >= H) r0 = -1;
    if (y == 1 && ty == 0) r1 = 0;
    if (y == H - 2 && ty == 2) r1 = H - 1;
    if (c0 < 0 || c0 >= W) c0 = -1;
    if (x == 1 && tx == 0) c1 = 0;
    if (x == W - 2 && tx == 2) c1 = W - 1;
    if (r0 >= 0 && c0 >= 0) d.o0 = r0 * OW + c0;
    if (r0 >= 0 && c1 >= 0) d.o1 = r0 * OW + c1;
    if (r1 >= 0 && c0 >= 0) d.o2 = r1 * OW + c0;
    if (r1 >= 0 && c1 >= 0) d.o3 = r1 * OW + c1;
    return d;
}
__device__ __forceinline__ float dy_sum(const float* q, const DyOffs& d) {
    float s = 0.f;
    if (d.o0 >= 0) s += q[d.o0];
    if (d.o1 >= 0) s += q[d.o1];
    if (d.o2 >= 0) s += q[d.o2];
    if (d.o3 >= 0) s += q[d.o3];
    return s;
}

struct InPixKSt {
    InPixSt px;
    int kc;
};

__device__ __forceinline__ InPixSt in_pix(int p, int Npix, int H, int W) {
    InPixSt px;
    px.valid = p < Npix;
    int hw = H * W;
    px.img = p / hw;
    int pix = p - px.img * hw;
    px.y = pix / W;
    px.x = pix - px.y * W;
    return px;
}

template <int KH>
struct DgradB {  // B[k=(co,dy,dx)][n=input pixel]
    static constexpr bool ALONG_K = false;
    typedef InPixKSt St;
    const float* dy;
    int K, Npix, H, W, Cout, OH, OW, stride, pad, reflect;
    __device__ __forceinline__ void init(St& st, int p) const { st = St{in_pix(p, Npix, H, W), 0}; }
    __device__ __forceinline__ void chunk(St& st, int kc) const { st.kc = kc; }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const int k = st.kc + kl;
        if (!st.px.valid || k >= K) return 0.f;
        int co = k / (KH * KH);
        int tap = k - co * (KH * KH);
        int ty = tap / KH, tx = tap - ty * KH;
        const float* d = dy + (size_t)(st.px.img * Cout + co) * OH * OW;
        return dy_sum(d, dy_offsets(st.px.y, st.px.x, ty, tx, H, W, OH, OW, stride, pad, reflect));
    }
};

struct DgradEpi {  // dx[img][ci][pix] (= or +=) acc
    typedef size_t St;
    float* dx;
    int Cin, HW, accumulate;
    unsigned* amax = nullptr;           // != nullptr: the patch kernels report max |dx as stored| here (the entry point's amax_dx)
    __device__ __forceinline__ St col(int p) const {
        int img = p / HW;
        return (size_t)img * Cin * HW + (p - img * HW);
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        float* q = dx + base + (size_t)m * HW;
        *q = accumulate ? (*q + v) : v;
    }
    __device__ __forceinline__ void put4(St base, int m, float4 v) const {
        float4* q = reinterpret_cast<float4*>(dx + base + (size_t)m * HW);
        if (accumulate) { const float4 o = *q; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        *q = v;
    }
    __device__ __forceinline__ float put_get(St base, int m, float v) const {       // put, returning the stored value
        float* q = dx + base + (size_t)m * HW;
        const float r = accumulate ? (*q + v) : v;
        *q = r;
        return r;
    }
    __device__ __forceinline__ float put4_get(St base, int m, float4 v) const {     // put4, returning the largest stored magnitude
        float4* q = reinterpret_cast<float4*>(dx + base + (size_t)m * HW);
        if (accumulate) { const float4 o = *q; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        *q = v;
        return fmaxf(fmaxf(jp_fmag(v.x), jp_fmag(v.y)), fmaxf(jp_fmag(v.z), jp_fmag(v.w)));
    }
};

// =============================================================== tap-major ("T") fast-path loaders
// packed weights wp[tap][row][Cp] (row = co for forward, ci for dgrad; Cp = reduction channels padded to 32)
struct PackASt {
    const float* base;   // wave-uniform: (tap, channel chunk) corner of the packed weights
    unsigned voff;       // per-lane byte offset: (row within the 8-row group, channel within the chunk)
};
struct PackA {  // A[m=row][k=(tap,c)] = wp[(tap*M + m)*Cp + c]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    typedef PackASt St;
    const float* wp;
    int M, Kp, Cp, khw;
    __device__ __forceinline__ void init(St& st, int, int) const {
        st.base = wp;
        st.voff = ((threadIdx.x >> 5) * Cp + (threadIdx.x & 31)) * 4u;
    }
    __device__ __forceinline__ void fix(St& st, int k) const {
        // K order = (channel chunk of 32, tap, channel in chunk): the 9 taps of one channel chunk are consecutive
        // K-chunks, so the gathered input rows are re-read while still hot in L1/L2 instead of from the fabric
        const int q = __builtin_amdgcn_readfirstlane(k >> 5);
        const int cc = q / khw, tap = q - cc * khw;
        st.base = wp + (size_t)tap * M * Cp + cc * 32;
    }
    // rows >= M are not masked: they read the next tap's rows (or the scratch slack after the last tap, see
    // jp_conv2d_ws_floats) and the epilogue never stores them.  Kp is a multiple of KC.
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)m_u * Cp;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};

struct FwdBTSt {
    int img_rel, iy0, ix0;   // per-lane: image relative to the block's first image, top-left tap coordinate
    int img0;                // uniform: image of the block's first pixel
    const float* rowp;       // uniform: plane (segment, img0, first channel of the chunk)
    unsigned voff;           // per-lane byte offset of (relative image, tap position) from rowp
    int hw, nm1;             // uniform: plane size of the segment; valid channels in this chunk - 1
    int ok;                  // per-lane, zero padding only: the tap lies inside the image
};

template <int KH, bool REFLECT>
struct FwdBT {  // B[k=(tap,ci)][n=pixel]
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef FwdBTSt St;
    Src3 src;
    int Cp, Npix, OH, OW, stride, pad;
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int ohw = OH * OW;
        p = min(p, Npix - 1);          // columns >= N are computed on a duplicate pixel and never stored
        const int img = p / ohw, pix = p - img * ohw;
        const int oy = pix / OW, ox = pix - oy * OW;
        st.img0 = min(p0, Npix - 1) / ohw;
        st.img_rel = img - st.img0;
        st.iy0 = oy * stride - pad;
        st.ix0 = ox * stride - pad;
        st.rowp = src.p0;
        st.voff = 0;
        st.hw = 0;
        st.nm1 = 0;
        st.ok = 1;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int q = kc >> 5;                 // chunk index = channel_chunk * taps + tap
        const int cc = q / (KH * KH), tap = q - cc * (KH * KH);
        const int ci0 = cc << 5;
        const int dy = tap / KH, dx = tap - dy * KH;
        int iy = st.iy0 + dy, ix = st.ix0 + dx;
        if (REFLECT) {
            iy = jp_reflect(iy, src.H);
            ix = jp_reflect(ix, src.W);
        } else {
            st.ok = (unsigned)iy < (unsigned)src.H && (unsigned)ix < (unsigned)src.W;
            iy = min(max(iy, 0), src.H - 1);
            ix = min(max(ix, 0), src.W - 1);
        }
        const bool a = ci0 < src.e0, b = ci0 < src.e1;   // segment ends are multiples of 32 (host-checked)
        const float* p = a ? src.p0 : (b ? src.p1 : src.p2);
        const int c0 = a ? 0 : (b ? src.e0 : src.e1);
        const int ce = a ? src.e0 : (b ? src.e1 : src.e2);
        const int sh = a ? src.s0 : (b ? src.s1 : src.s2);
        const int h = src.H >> sh, w = src.W >> sh, Cs = ce - c0;
        st.hw = h * w;
        st.voff = (unsigned)((st.img_rel * Cs * h + (iy >> sh)) * w + (ix >> sh)) * 4u;
        st.rowp = p + (size_t)(st.img0 * Cs + (ci0 - c0)) * st.hw;
        st.nm1 = min(32, ce - ci0) - 1;       // rows beyond are clamped: their packed weights are zero
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {   // kl is wave-uniform
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * st.hw;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return REFLECT || __all(st.ok); }
    __device__ __forceinline__ float post(const St& st, float v, int) const { return (REFLECT || st.ok) ? v : 0.f; }
};

struct DgradBTSt {
    int img_rel, y, x, img0;
    const float* rowp;   // uniform: dY plane (img0, first output channel of the chunk)
    unsigned voff;       // per-lane byte offset of (relative image, tap position)
    int nm1, ok;
};

// main dgrad gather: the single dY entry reached through tap (ty,tx) by the *direct* (non-folded) path.
// With reflection padding the extra folded-in entries of the 4 border-adjacent lines are added by a second,
// tiny launch (DgradBorderB below), which keeps this hot loop as lean as the forward gather.
template <int KH, bool S1 = false>   // S1: stride 1 (no per-lane integer divisions in the chunk prologue)
struct DgradBT {  // B[k=(tap,co)][n=input pixel]
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef DgradBTSt St;
    const float* dy;
    int Cp, Npix, H, W, Cout, OH, OW, stride, pad, reflect;
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int hw = H * W;
        p = min(p, Npix - 1);
        const int img = p / hw, pix = p - img * hw;
        st.y = pix / W;
        st.x = pix - st.y * W;
        st.img0 = min(p0, Npix - 1) / hw;
        st.img_rel = img - st.img0;
        st.rowp = dy;
        st.voff = 0;
        st.nm1 = 0;
        st.ok = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int q = kc >> 5;
        const int cc = q / (KH * KH), tap = q - cc * (KH * KH);
        const int co0 = cc << 5;
        const int ty = tap / KH, tx = tap - ty * KH;
        int oy, ox, ok;
        if (reflect) {   // 3x3 stride 1 pad 1: direct path = padded row y+1, dY row y+1-ty
            oy = st.y + 1 - ty;
            ox = st.x + 1 - tx;
            ok = 1;
        } else {
            const int ny = st.y + pad - ty, nx = st.x + pad - tx;
            if (S1) {
                oy = ny;
                ox = nx;
                ok = 1;        // range-checked below
            } else {
                oy = ny / stride;
                ox = nx / stride;
                ok = ny >= 0 && nx >= 0 && oy * stride == ny && ox * stride == nx;
            }
        }
        st.ok = ok && (unsigned)oy < (unsigned)OH && (unsigned)ox < (unsigned)OW;
        oy = min(max(oy, 0), OH - 1);
        ox = min(max(ox, 0), OW - 1);
        const int ohw = OH * OW;
        st.voff = (unsigned)(st.img_rel * Cout * ohw + oy * OW + ox) * 4u;
        st.rowp = dy + (size_t)(st.img0 * Cout + co0) * ohw;
        st.nm1 = min(32, Cout - co0) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {   // kl is wave-uniform
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * (OH * OW);
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok); }
    __device__ __forceinline__ float post(const St& st, float v, int) const { return st.ok ? v : 0.f; }
};

// ---- B loader of the row-tile kernel (igemm.h jp_igemm_r3_kernel): 3x3 stride 1 pad 1, the pixel tile is BN consecutive
// pixels of ONE image row.  REV = dgrad (row y+1-ty of dY, taps mirrored, zero fill -- the reflection fold is the border
// pass's job); otherwise forward with reflection or zero padding.  Sources must be stored at full resolution.
struct FwdBR3St {
    int img, y, x0;          // uniform: the tile's image, row, first column
    const float* rowp;       // uniform: (segment, image, first channel of the chunk, source row, x0)
    int hw, nm1, rowok;      // uniform
};
template <bool REFLECT, bool REV, int BN>
struct FwdBR3 {
    static constexpr bool REVERSE = REV;
    typedef FwdBR3St St;
    Src3 src;
    int H, W;
    __device__ __forceinline__ void init(St& st, int n0) const {
        const int hw = H * W;
        st.img = n0 / hw;
        const int rem = n0 - st.img * hw;
        st.y = rem / W;
        st.x0 = rem - st.y * W;
        st.rowp = src.p0;
        st.hw = hw;
        st.nm1 = 0;
        st.rowok = 0;
    }
    __device__ __forceinline__ void row(St& st, int kc) const {
        const int q = kc >> 5;
        const int cc = q / 9, tap = q - cc * 9;
        const int dy = tap / 3;
        int iy = REV ? st.y + 1 - dy : st.y - 1 + dy;
        if (REFLECT) {
            iy = jp_reflect(iy, H);
            st.rowok = 1;
        } else {
            st.rowok = (unsigned)iy < (unsigned)H;
            iy = min(max(iy, 0), H - 1);
        }
        const int ci0 = cc << 5;
        const bool a = ci0 < src.e0, b = ci0 < src.e1;
        const float* p = a ? src.p0 : (b ? src.p1 : src.p2);
        const int c0 = a ? 0 : (b ? src.e0 : src.e1);
        const int ce = a ? src.e0 : (b ? src.e1 : src.e2);
        st.rowp = p + ((size_t)(st.img * (ce - c0) + (ci0 - c0)) * H + iy) * W + st.x0;
        st.nm1 = min(32, ce - ci0) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int n_l) const {    // kl wave-uniform, n_l = lane's column
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * st.hw;
        const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + (unsigned)n_l * 4u);
        return st.rowok ? v : 0.f;
    }
    __device__ __forceinline__ float halo(const St& st, int kl, int side) const {   // column x0-1 / x0+BN
        int x = side ? st.x0 + BN : st.x0 - 1;
        bool ok = st.rowok;
        if (REFLECT) x = jp_reflect(x, W);
        else { ok = ok && (unsigned)x < (unsigned)W; x = min(max(x, 0), W - 1); }
        const float v = st.rowp[(size_t)min(kl, st.nm1) * st.hw + (x - st.x0)];
        return ok ? v : 0.f;
    }
};

// ---- Few input channels (the 7x7 stride-2 ResNet stems: 3 image channels, 6 for the pose pair): K = (tap, c) with the
// channels padded to CP = 4 or 8, so a K chunk of 32 holds 32/CP whole taps; one per-lane offset per tap per chunk,
// every element a scalar-base load (the generic path decodes (c, dy, dx) per element).  64x256 tiles only (Cout <= 64).
struct PackARowSt {
    const float* base;
    unsigned voff;
};
struct PackARow {  // A[m][k] = wp[m*Kp + k]  (row-major, K zero-padded to Kp)
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    typedef PackARowSt St;
    const float* wp;
    int Kp;
    __device__ __forceinline__ void init(St& st, int, int) const {
        st.base = wp;
        st.voff = ((threadIdx.x >> 5) * Kp + (threadIdx.x & 31)) * 4u;
    }
    __device__ __forceinline__ void fix(St& st, int k) const { st.base = wp + __builtin_amdgcn_readfirstlane(k & ~31); }
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)m_u * Kp;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};
template <int TPC>
struct FwdBCSt {
    int img_rel, iy0, ix0, img0;
    unsigned voff[TPC];
    unsigned ok;
};
template <int KH, int CP>
struct FwdBC {  // B[k=(tap, c)][n=pixel], zero padding, single full-resolution source
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    static constexpr int TPC = 32 / CP;
    typedef FwdBCSt<TPC> St;
    const float* x;
    int Cin, H, W, Npix, OH, OW, stride, pad;
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int ohw = OH * OW;
        p = min(p, Npix - 1);
        const int img = p / ohw, pix = p - img * ohw;
        const int oy = pix / OW, ox = pix - oy * OW;
        st.img0 = min(p0, Npix - 1) / ohw;
        st.img_rel = img - st.img0;
        st.iy0 = oy * stride - pad;
        st.ix0 = ox * stride - pad;
        st.ok = 0;
#pragma unroll
        for (int s = 0; s < TPC; ++s) st.voff[s] = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int tap0 = (kc >> 5) * TPC;
        unsigned ok = 0;
#pragma unroll
        for (int s = 0; s < TPC; ++s) {
            const int tap = min(tap0 + s, KH * KH - 1);     // taps past the filter: zero weights
            const int dy = tap / KH, dx = tap - dy * KH;
            int iy = st.iy0 + dy, ix = st.ix0 + dx;
            ok |= (unsigned)((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) << s;
            iy = min(max(iy, 0), H - 1);
            ix = min(max(ix, 0), W - 1);
            st.voff[s] = (unsigned)((st.img_rel * Cin * H + iy) * W + ix) * 4u;
        }
        st.ok = ok;
    }
    // 64x256 tile: the k row of slot r is r itself -> tap slot r/CP, channel r%CP at compile time
    __device__ __forceinline__ float get(const St& st, int, int r) const {
        const float* rp = x + ((size_t)st.img0 * Cin + min(r % CP, Cin - 1)) * H * W;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff[r / CP]);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok == ((1u << TPC) - 1u)); }
    __device__ __forceinline__ float post(const St& st, float v, int r) const { return ((st.ok >> (r / CP)) & 1u) ? v : 0.f; }
};

// ---- Upsample-aware 3x3 reflect conv (iconv layers: cat(reduce, up2x(x), disp), depth_decoder.py:68,76-77).
// For the nearest-2x upsampled segment U = up(X) an output pixel (2i+a, 2j+b) sees only a 2x2 patch of X through its
// 9 taps: rows {i-1+a, i+a} x cols {j-1+b, j+b} (reflection padding of U == edge clamp on X).  Output pixels are
// enumerated parity-class-major n = (class (a,b), img, i, j) so a tile is class-uniform; the K loop then runs 9 taps
// over the full-resolution segments but only 4 slots (r, s) over the upsampled one, against weights pre-summed per
// class:  W'_{ab}[r][s] = sum_{dy in Dy(a,r)} sum_{dx in Dx(b,s)} W[dy][dx],  Dy(0,.) = {0},{1,2}; Dy(1,.) = {0,1},{2}.
// 27.7 % fewer MFMA FLOPs on the 513-channel layers.
struct ParSeg {       // K-chunk layout of the three channel segments
    int q0, q1;       // cumulative chunk counts after segment 0 / 1
    int t0, t1, t2;   // taps (9) or slots (4) per channel chunk of each segment
    int o0, o1, o2;   // float offset of each segment's packed weights in ws
    int p0, p1, p2;   // padded channel count (row length) of each segment
};
struct PackAPSt {
    const float* base;
    unsigned rg, cl, Cp;   // row group (t>>5), channel in chunk (t&31), row length of the current segment
    int cls;
};
struct PackAP {   // A[m=co][k] for the segment-piecewise K order; up segments hold [class][slot][co][Cp]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool WANTS_TILE = true;
    typedef PackAPSt St;
    const float* wp;
    ParSeg ps;
    int M, Nc;
    __device__ __forceinline__ void init(St& st, int, int, int, int n0) const {
        st.base = wp;
        st.rg = threadIdx.x >> 5;
        st.cl = threadIdx.x & 31;
        st.Cp = 32;
        st.cls = n0 / Nc;
    }
    __device__ __forceinline__ void fix(St& st, int k) const {
        const int q = __builtin_amdgcn_readfirstlane(k >> 5);
        const bool a = q < ps.q0, b = q < ps.q1;
        const int ql = a ? q : (b ? q - ps.q0 : q - ps.q1);
        const int T = a ? ps.t0 : (b ? ps.t1 : ps.t2);
        const int off = a ? ps.o0 : (b ? ps.o1 : ps.o2);
        const int Cp = a ? ps.p0 : (b ? ps.p1 : ps.p2);
        const int cc = ql / T, t = ql - cc * T;
        const int plane = T == 4 ? st.cls * 4 + t : t;      // [class][slot] or [tap]
        st.base = wp + off + (size_t)plane * M * Cp + cc * 32;
        st.Cp = Cp;
    }
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)m_u * st.Cp;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + (st.rg * st.Cp + st.cl) * 4u);
    }
};

struct FwdBPSt {
    int img_rel, i, j, img0, a, b;
    const float* rowp;
    unsigned voff;
    int hw, nm1;
};
struct FwdBP {  // B[k][n=(class, img, i, j)], 3x3 stride 1 reflection pad
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef FwdBPSt St;
    Src3 src;
    ParSeg ps;
    int Nc, h2, w2;    // pixels per class, half-resolution size
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int cls = p0 / Nc;
        st.a = cls >> 1;
        st.b = cls & 1;
        const int hw2 = h2 * w2;
        const int q = min(p - cls * Nc, Nc - 1), q0 = p0 - cls * Nc;
        const int img = q / hw2, pix = q - img * hw2;
        st.i = pix / w2;
        st.j = pix - st.i * w2;
        st.img0 = q0 / hw2;
        st.img_rel = img - st.img0;
        st.rowp = src.p0;
        st.voff = 0;
        st.hw = 0;
        st.nm1 = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int q = kc >> 5;
        const bool sa = q < ps.q0, sb = q < ps.q1;
        const int ql = sa ? q : (sb ? q - ps.q0 : q - ps.q1);
        const int T = sa ? ps.t0 : (sb ? ps.t1 : ps.t2);
        const float* p = sa ? src.p0 : (sb ? src.p1 : src.p2);
        const int Cs = sa ? src.e0 : (sb ? src.e1 - src.e0 : src.e2 - src.e1);
        const int cc = ql / T, t = ql - cc * T;
        int yy, xx, h, w;
        if (T == 4) {      // upsampled segment: 2x2 patch of the half-resolution tensor, edge-clamped
            h = h2; w = w2;
            yy = min(max(st.i - 1 + st.a + (t >> 1), 0), h2 - 1);
            xx = min(max(st.j - 1 + st.b + (t & 1), 0), w2 - 1);
        } else {           // full-resolution segment: the usual 9 reflected taps
            h = 2 * h2; w = 2 * w2;
            const int dy = t / 3, dx = t - dy * 3;
            yy = jp_reflect(2 * st.i + st.a - 1 + dy, h);
            xx = jp_reflect(2 * st.j + st.b - 1 + dx, w);
        }
        st.hw = h * w;
        st.voff = (unsigned)((st.img_rel * Cs * h + yy) * w + xx) * 4u;
        st.rowp = p + (size_t)(st.img0 * Cs + cc * 32) * st.hw;
        st.nm1 = min(32, Cs - cc * 32) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * st.hw;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St&) const { return true; }
    __device__ __forceinline__ float post(const St&, float v, int) const { return v; }
};
struct FwdEpiP {  // y[img][co][2i+a][2j+b] = act(acc + bias[co])
    typedef size_t St;
    float* y;
    const float* bias;
    int Cout, Nc, h2, w2, act;
    __device__ __forceinline__ St col(int n) const {
        const int cls = n / Nc, q = n - cls * Nc;
        const int hw2 = h2 * w2;
        const int img = q / hw2, pix = q - img * hw2;
        const int i = pix / w2, j = pix - i * w2;
        return (size_t)img * Cout * (4 * hw2) + (size_t)(2 * i + (cls >> 1)) * (2 * w2) + 2 * j + (cls & 1);
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        if (bias) v += bias[m];
        y[base + (size_t)m * (4 * h2 * w2)] = jp_act(v, act);
    }
};


// ---- dgrad of the upsampled segment, directly at half resolution:
//   dX[c][i][j] = sum_{class (a,b), slot (r,s), co} W'_{ab}[r][s][co][c] * dY[co][2i'+a][2j'+b],
//   (i', j') = (i+1-a-r, j+1-b-s) where it exists (GEMM M=c, N=half-res pixels, K=(co chunk, 16 (class,slot), co); 4/9 of
//   the full-resolution dgrad + 2x2 sum it replaces).  The edge clamp of the forward adds, on the 4 boundary lines, the
//   entries (i'=0 via a=0,r=0 | i'=h-1 via a=1,r=1, same for columns): a split-K border pass like the reflection one.
struct DgradUPSt {
    int img_rel, i, j, img0;
    const float* rowp;
    unsigned voff;
    int nm1, ok;
};
struct DgradUPB {
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef DgradUPSt St;
    const float* dy;
    int Npix2, h2, w2, Cout;
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int hw2 = h2 * w2;
        p = min(p, Npix2 - 1);
        const int img = p / hw2, pix = p - img * hw2;
        st.i = pix / w2;
        st.j = pix - st.i * w2;
        st.img0 = min(p0, Npix2 - 1) / hw2;
        st.img_rel = img - st.img0;
        st.rowp = dy;
        st.voff = 0;
        st.nm1 = 0;
        st.ok = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int qk = kc >> 5;
        const int cc = qk >> 4, q = qk & 15;
        const int a = q >> 3, b = (q >> 2) & 1, r = (q >> 1) & 1, s = q & 1;
        const int co0 = cc << 5;
        int ip = st.i + 1 - a - r, jp = st.j + 1 - b - s;
        st.ok = (unsigned)ip < (unsigned)h2 && (unsigned)jp < (unsigned)w2;
        ip = min(max(ip, 0), h2 - 1);
        jp = min(max(jp, 0), w2 - 1);
        const int HW = 4 * h2 * w2;
        st.voff = (unsigned)(st.img_rel * Cout * HW + (2 * ip + a) * (2 * w2) + 2 * jp + b) * 4u;
        st.rowp = dy + (size_t)(st.img0 * Cout + co0) * HW;
        st.nm1 = min(32, Cout - co0) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * (4 * h2 * w2);
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok); }
    __device__ __forceinline__ float post(const St& st, float v, int) const { return st.ok ? v : 0.f; }
};

// boundary pixels of the half-resolution map: rows 0 / h-1, columns 0 / w-1 (duplicates masked)
__device__ __forceinline__ InPixSt edge_pix(int b, int Nb, int h, int w) {
    InPixSt px;
    const int per = 2 * w + 2 * h;
    px.valid = b < Nb;
    px.img = b / per;
    const int i = b - px.img * per;
    int y, x;
    bool dup = false;
    if (i < w) { y = 0; x = i; }
    else if (i < 2 * w) { y = h - 1; x = i - w; dup = (h == 1); }
    else if (i < 2 * w + h) { y = i - 2 * w; x = 0; dup = (y == 0 || y == h - 1); }
    else { y = i - 2 * w - h; x = w - 1; dup = (y == 0 || y == h - 1) || (w == 1); }
    px.y = y; px.x = x;
    if (dup) px.valid = 0;
    return px;
}
struct DgradUPBorderSt {
    InPixSt px;
    const float* p;
    int o1, o2, o3, n;
};
struct DgradUPBorderB {   // only the clamp-folded entries: (extra row, any column) and (regular row, extra column)
    static constexpr bool ALONG_K = false;
    typedef DgradUPBorderSt St;
    const float* dy;
    int Nb, h2, w2, Cout;
    __device__ __forceinline__ void init(St& st, int b) const { st = St{edge_pix(b, Nb, h2, w2), nullptr, -1, -1, -1, 0}; }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int qk = kc >> 5;
        const int cc = qk >> 4, q = qk & 15;
        const int a = q >> 3, b = (q >> 2) & 1, r = (q >> 1) & 1, s = q & 1;
        const int co0 = cc << 5;
        st.n = 0;
        if (!st.px.valid || co0 >= Cout) return;
        const int i = st.px.y, j = st.px.x;
        const int er = (i == 0 && a == 0 && r == 0) ? 0 : ((i == h2 - 1 && a == 1 && r == 1) ? h2 - 1 : -1);
        const int ec = (j == 0 && b == 0 && s == 0) ? 0 : ((j == w2 - 1 && b == 1 && s == 1) ? w2 - 1 : -1);
        if (er < 0 && ec < 0) return;
        const int rr = i + 1 - a - r, rc = j + 1 - b - s;
        const bool rrv = (unsigned)rr < (unsigned)h2, rcv = (unsigned)rc < (unsigned)w2;
        const int W = 2 * w2;
        st.o1 = (er >= 0 && rcv) ? (2 * er + a) * W + 2 * rc + b : -1;
        st.o2 = (rrv && ec >= 0) ? (2 * rr + a) * W + 2 * ec + b : -1;
        st.o3 = (er >= 0 && ec >= 0) ? (2 * er + a) * W + 2 * ec + b : -1;
        st.p = dy + (size_t)(st.px.img * Cout + co0) * (4 * h2 * w2);
        st.n = min(32, Cout - co0);
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        if (kl >= st.n) return 0.f;
        const float* q = st.p + (size_t)kl * (4 * h2 * w2);
        float v = 0.f;
        if (st.o1 >= 0) v += q[st.o1];
        if (st.o2 >= 0) v += q[st.o2];
        if (st.o3 >= 0) v += q[st.o3];
        return v;
    }
    // slots (a, b, r, s) that fold something in for some pixel of the tile (see chunk()); the rest are stepped over
    static constexpr bool SKIP = true;
    __device__ __forceinline__ unsigned tile_mask(const St& st) const {
        __shared__ unsigned tm;
        if (threadIdx.x == 0) tm = 0;
        __syncthreads();
        unsigned mine = 0;
        if (st.px.valid) {
            const int i = st.px.y, j = st.px.x;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int a = q >> 3, b = (q >> 2) & 1, r = (q >> 1) & 1, s2 = q & 1;
                const bool er = (i == 0 && a == 0 && r == 0) || (i == h2 - 1 && a == 1 && r == 1);
                const bool ec = (j == 0 && b == 0 && s2 == 0) || (j == w2 - 1 && b == 1 && s2 == 1);
                if (er || ec) mine |= 1u << q;
            }
        }
        if (mine) atomicOr(&tm, mine);
        __syncthreads();
        return (unsigned)__builtin_amdgcn_readfirstlane((int)tm);
    }
    __device__ __forceinline__ bool skip(unsigned m, int kc) const { return !((m >> ((kc >> 5) & 15)) & 1u); }
};
struct DgradEdgeEpi {  // dx[img][c][y][x] += acc for the boundary pixel b of a (h, w) map
    typedef long St;
    float* dx;
    int C, h, w, Nb, split;
    __device__ __forceinline__ St col(int b) const {
        const InPixSt px = edge_pix(b, Nb, h, w);
        return px.valid ? (long)px.img * C * h * w + px.y * w + px.x : -1;
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        if (base < 0) return;
        float* q = dx + base + (size_t)m * h * w;
        if (split) atomicAdd(q, v);       // split-K partials meet here
        else *q += v;                     // one workgroup owns the pixel: plain read-modify-write
    }
};

// ---- 3x3 stride-2 pad-1 dgrad (ResNet downsampling convs), parity-class form.  An input pixel (y, x) is reached only
// through taps with ty = y+1 (mod 2), tx = x+1 (mod 2): 1, 2, 2 or 4 of the 9.  Input pixels are enumerated class-major
// n = (class (py,px), img, i, j) with y = 2i+py, x = 2j+px, so a pixel tile is class-uniform and the K loop runs over
// 4 tap slots (r, s) instead of 9 taps; slots a class does not have are masked.  (H, W even; class size % 256 == 0.)
struct PackAS2St {
    const float* base;
    unsigned voff;
    int py, px;
};
struct PackAS2 {   // A[m=ci][k=(cc, slot, c)] = wp[(tap(slot, class)*M + m)*Cp + c]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool WANTS_TILE = true;
    typedef PackAS2St St;
    const float* wp;
    int M, Cp, Nc;   // Nc = pixels per class
    __device__ __forceinline__ void init(St& st, int, int, int, int n0) const {
        st.base = wp;
        st.voff = ((threadIdx.x >> 5) * Cp + (threadIdx.x & 31)) * 4u;
        const int cls = n0 / Nc;
        st.py = cls >> 1;
        st.px = cls & 1;
    }
    __device__ __forceinline__ void fix(St& st, int k) const {
        const int q = __builtin_amdgcn_readfirstlane(k >> 5);
        const int cc = q >> 2, r = (q >> 1) & 1, c = q & 1;
        const int ty = st.py ? 2 * r : 1, tx = st.px ? 2 * c : 1;   // masked slots read a valid (unused) tap
        st.base = wp + (size_t)(ty * 3 + tx) * M * Cp + cc * 32;
    }
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)m_u * Cp;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};

struct DgradS2St {
    int img_rel, i, j, img0, py, px;
    const float* rowp;
    unsigned voff;
    int nm1, ok;
};
struct DgradS2B {  // B[k=(cc, slot, co)][n=(class, img, i, j)]
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef DgradS2St St;
    const float* dy;
    int Cp, Nc, H2, W2, Cout, OH, OW;
    __device__ __forceinline__ void init(St& st, int p, int p0) const {
        const int cls = p0 / Nc;                 // tile-uniform
        st.py = cls >> 1;
        st.px = cls & 1;
        const int hw2 = H2 * W2;
        const int q = min(p - cls * Nc, Nc - 1), q0 = p0 - cls * Nc;
        const int img = q / hw2, pix = q - img * hw2;
        st.i = pix / W2;
        st.j = pix - st.i * W2;
        st.img0 = q0 / hw2;
        st.img_rel = img - st.img0;
        st.rowp = dy;
        st.voff = 0;
        st.nm1 = 0;
        st.ok = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int q = kc >> 5;
        const int cc = q >> 2, r = (q >> 1) & 1, c = q & 1;
        const int co0 = cc << 5;
        // odd rows: taps 0 and 2 -> dY rows i+1 and i; even rows: tap 1 -> dY row i (slot r = 1 does not exist)
        int oy = st.i + st.py - r, ox = st.j + st.px - c;
        st.ok = (st.py || r == 0) && (st.px || c == 0) && oy < OH && ox < OW;
        oy = min(max(oy, 0), OH - 1);
        ox = min(max(ox, 0), OW - 1);
        const int ohw = OH * OW;
        st.voff = (unsigned)(st.img_rel * Cout * ohw + oy * OW + ox) * 4u;
        st.rowp = dy + (size_t)(st.img0 * Cout + co0) * ohw;
        st.nm1 = min(32, Cout - co0) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const float* rp = st.rowp + (size_t)min(kl, st.nm1) * (OH * OW);
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok); }
    __device__ __forceinline__ float post(const St& st, float v, int) const { return st.ok ? v : 0.f; }
};
struct DgradS2Epi {  // dx[img][ci][2i+py][2j+px] (= or +=) acc
    typedef size_t St;
    float* dx;
    int Cin, Nc, H2, W2, accumulate;
    __device__ __forceinline__ St col(int n) const {
        const int cls = n / Nc, q = n - cls * Nc;
        const int hw2 = H2 * W2;
        const int img = q / hw2, pix = q - img * hw2;
        const int i = pix / W2, j = pix - i * W2;
        return (size_t)img * Cin * (4 * hw2) + (size_t)(2 * i + (cls >> 1)) * (2 * W2) + 2 * j + (cls & 1);
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        float* q = dx + base + (size_t)m * (4 * H2 * W2);
        *q = accumulate ? (*q + v) : v;
    }
};

struct DgradS2PointEpi {  // dgrad of a 1x1 stride-2 conv: dx[img][ci][2i][2j] (= or +=) acc, the other three pixels of the 2x2 cell = 0
    typedef size_t St;
    float* dx;
    int Cin, ohw, OW, accumulate;
    __device__ __forceinline__ St col(int p) const {
        const int img = p / ohw, pix = p - img * ohw;
        const int i = pix / OW, j = pix - i * OW;
        return (size_t)img * Cin * (4 * ohw) + (size_t)(2 * i) * (2 * OW) + 2 * j;
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        float* q = dx + base + (size_t)m * (4 * ohw);
        if (accumulate) { *q += v; return; }
        *reinterpret_cast<float2*>(q) = make_float2(v, 0.f);
        *reinterpret_cast<float2*>(q + 2 * OW) = make_float2(0.f, 0.f);
    }
};

// Border pass of the reflection-pad adjoint.  N enumerates the 2W+2H border-adjacent pixels of every image
// (rows 1 and H-2, columns 1 and W-2; duplicates masked); the gather returns only the folded-in ("extra")
// dY entries: row extras r1 = 0 (y==1, ty==0) / H-1 (y==H-2, ty==2), column extras likewise.
struct DgradBorderSt {
    InPixSt px;
    int img0;
    const float* rowp;
    unsigned v1, v2, v3;
    float m1, m2, m3;
    int nm1;
};
__device__ __forceinline__ InPixSt border_pix(int b, int Nb, int H, int W) {
    InPixSt px;
    const int per = 2 * W + 2 * H;
    px.valid = b < Nb;
    px.img = b / per;
    const int i = b - px.img * per;
    int y, x;
    bool dup = false;
    if (i < W) { y = 1; x = i; }
    else if (i < 2 * W) { y = H - 2; x = i - W; dup = (H - 2 == 1); }
    else if (i < 2 * W + H) { y = i - 2 * W; x = 1; dup = (y == 1 || y == H - 2); }
    else { y = i - 2 * W - H; x = W - 2; dup = (y == 1 || y == H - 2) || (W - 2 == 1); }
    px.y = y; px.x = x;
    if (dup) px.valid = 0;
    return px;
}

template <int KH>
struct DgradBorderB {   // scalar-base: uniform dY plane pointer + three per-lane byte offsets with 0/1 weights, no branches
    static constexpr bool ALONG_K = false;
    static constexpr bool POST = true;
    typedef DgradBorderSt St;
    const float* dy;
    int Cp, Nb, H, W, Cout;
    __device__ __forceinline__ void init(St& st, int b, int b0) const {
        st.px = border_pix(min(b, Nb - 1), Nb, H, W);
        if (b >= Nb) st.px.valid = 0;
        st.img0 = border_pix(min(b0, Nb - 1), Nb, H, W).img;
        st.rowp = dy;
        st.v1 = st.v2 = st.v3 = 0;
        st.m1 = st.m2 = st.m3 = 0.f;
        st.nm1 = 0;
    }
    __device__ __forceinline__ void chunk(St& st, int kc) const {
        const int q = kc >> 5;
        const int cc = q / (KH * KH), tap = q - cc * (KH * KH);
        const int co0 = cc << 5;
        const int ty = tap / KH, tx = tap - ty * KH;
        const DyOffs d = dy_offsets(st.px.y, st.px.x, ty, tx, H, W, H, W, 1, 1, 1);
        const bool ok = st.px.valid;
        const unsigned base = (unsigned)((st.px.img - st.img0) * Cout * H * W);
        st.m1 = (ok && d.o1 >= 0) ? 1.f : 0.f;
        st.m2 = (ok && d.o2 >= 0) ? 1.f : 0.f;
        st.m3 = (ok && d.o3 >= 0) ? 1.f : 0.f;
        st.v1 = (base + (unsigned)max(d.o1, 0)) * 4u;
        st.v2 = (base + (unsigned)max(d.o2, 0)) * 4u;
        st.v3 = (base + (unsigned)max(d.o3, 0)) * 4u;
        st.rowp = dy + (size_t)(st.img0 * Cout + co0) * H * W;
        st.nm1 = min(32, Cout - co0) - 1;
    }
    __device__ __forceinline__ float get(const St& st, int kl, int) const {
        const char* rp = reinterpret_cast<const char*>(st.rowp + (size_t)min(kl, st.nm1) * H * W);
        const float a = *reinterpret_cast<const float*>(rp + st.v1);
        const float b = *reinterpret_cast<const float*>(rp + st.v2);
        const float c = *reinterpret_cast<const float*>(rp + st.v3);
        return fmaf(st.m1, a, fmaf(st.m2, b, st.m3 * c));
    }
    __device__ __forceinline__ float post(const St&, float v, int) const { return v; }
    // Only the taps that fold something in are non-zero: (ty, tx) with a row extra at ty (y == 1 / H-2) or a column
    // extra at tx (x == 1 / W-2).  A pixel tile lies along one edge, so it needs 3 of the 9 taps (5 next to a corner):
    // the engine steps over the other K chunks.
    static constexpr bool SKIP = true;
    __device__ __forceinline__ unsigned tile_mask(const St& st) const {
        __shared__ unsigned tm;
        if (threadIdx.x == 0) tm = 0;
        __syncthreads();
        unsigned mine = 0;
        if (st.px.valid) {
            const unsigned ry = (st.px.y == 1 ? 1u : 0u) | (st.px.y == H - 2 ? 4u : 0u);
            const unsigned cx = (st.px.x == 1 ? 1u : 0u) | (st.px.x == W - 2 ? 4u : 0u);
#pragma unroll
            for (int ty = 0; ty < KH; ++ty)
#pragma unroll
                for (int tx = 0; tx < KH; ++tx)
                    if (((ry >> ty) | (cx >> tx)) & 1u) mine |= 1u << (ty * KH + tx);
        }
        if (mine) atomicOr(&tm, mine);
        __syncthreads();
        return (unsigned)__builtin_amdgcn_readfirstlane((int)tm);
    }
    __device__ __forceinline__ bool skip(unsigned m, int kc) const { return !((m >> ((kc >> 5) % (KH * KH))) & 1u); }
};

// Split policy of the border passes.  Their cost is the scattered read-modify-write of the epilogue (one 4-byte access per
// 64-byte sector, atomics when K is split: 12.6 M atomics = 0.24 ms for a 256-channel 256x256 layer with 6 splits), not
// the K loop -- so K is split only when the pass would otherwise be a few dozen workgroups.
static inline int border_splits(long btiles, int chunks) {
    if (btiles >= 48) return 1;
    return (int)std::max<long>(1, std::min<long>(jp_cdiv(96, btiles), chunks / 4));
}

struct DgradBorderEpi {  // dx[img][ci][y][x] += acc for the border pixel b
    typedef long St;
    float* dx;
    int Cin, H, W, Nb, split;
    __device__ __forceinline__ St col(int b) const {
        const InPixSt px = border_pix(b, Nb, H, W);
        return px.valid ? (long)px.img * Cin * H * W + px.y * W + px.x : -1;
    }
    __device__ __forceinline__ void put(St base, int m, float v) const {
        if (base < 0) return;
        float* q = dx + base + (size_t)m * H * W;
        if (split) atomicAdd(q, v);       // split-K partials meet here
        else *q += v;                     // one workgroup owns the pixel: plain read-modify-write
    }
};

// border pass through scratch: the K loop is split into slices that store part[slice][ci][b] (coalesced along the border pixels),
// then ONE small pass folds the slices into dx in a fixed order -- more workgroups on a launch that has only a few dozen tiles,
// the scattered read-modify-write done once, no atomics
// amax != nullptr: max |final value| of the pixels this pass touches goes to the slot the main pass reported into -- every element of dx
// is then covered by one of the two (an upper bound: the main pass's value of a border pixel is in there as well)
__global__ void border_add_kernel(const float* __restrict__ part, float* __restrict__ dx, int Cin, int Nb, int H, int W,
                                  int slices, unsigned* __restrict__ amax) {
    const long total = (long)Cin * Nb;
    float mx = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / Nb), b = (int)(i - (long)m * Nb);
        const InPixSt px = border_pix(b, Nb, H, W);
        if (!px.valid) continue;
        float s = 0.f;
        for (int k = 0; k < slices; ++k) s += part[(size_t)k * total + i];
        float* q = dx + ((size_t)px.img * Cin + m) * H * W + px.y * W + px.x;
        const float r = *q + s;
        *q = r;
        mx = fmaxf(mx, jp_fmag(r));
    }
    jp_wave_amax_commit(mx, amax);
}

// the same fold for the edge pass of an upsampled segment (boundary pixels of the half-resolution map, edge_pix)
__global__ void edge_add_kernel(const float* __restrict__ part, float* __restrict__ dx, int C, int Nb, int h, int w, int slices) {
    const long total = (long)C * Nb;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / Nb), b = (int)(i - (long)m * Nb);
        const InPixSt px = edge_pix(b, Nb, h, w);
        if (!px.valid) continue;
        float s = 0.f;
        for (int k = 0; k < slices; ++k) s += part[(size_t)k * total + i];
        dx[((size_t)px.img * C + m) * h * w + px.y * w + px.x] += s;
    }
}

template <int WM, int WN, class A, class B, class E>
void launch_r3(A a, B b, E e, int M, int N, int K, hipStream_t st) {
    dim3 grid(N / (64 * WN), jp_cdiv(M, 64 * WM), 1);
    jp_prof_before(__PRETTY_FUNCTION__, 2.0 * M * (double)N * K, st);
    hipLaunchKernelGGL((jp_igemm_r3_kernel<WM, WN, KC, A, B, E>), grid, dim3(256), 0, st, a, b, e, M, N, K);
    jp_prof_after(st);
}

// P9 patch kernel (igemm_p9.h): 3x3 stride 1 pad 1, single full-resolution source.  JP_P9=0 in the environment turns
// it off (A/B measurements); the pack needs p9_ws_floats() floats of scratch.
inline bool p9_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9"); return e ? atoi(e) : 1; }();
    return on != 0;
}
inline bool p9u_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9U"); return e ? atoi(e) : 1; }();
    return on != 0;
}
template <class E>
const char* p9u_tag() { return __PRETTY_FUNCTION__; }
inline bool p9us_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9US"); return e ? atoi(e) : 1; }();
    return on != 0;
}
template <class E>
const char* p9us2_tag() { return __PRETTY_FUNCTION__; }
// P9SD (igemm_p9sd.h): dgrad of the upsampled iconv segment at half resolution on the bf16 pipe; JP_P9SD=0 keeps DgradUPB
inline bool p9sd_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9SD"); return e ? atoi(e) : 1; }();
    return on != 0;
}
inline long p9sd_floats(int rows, int Cout) { return (long)jp_cdiv(rows, 128) * ((long)((Cout + 31) / 32 * 2) * 16 + P9S_AHEAD) * (JP_NS * 1024) + JP_PACK_HDR; }
template <class E>
const char* p9sd_tag() { return __PRETTY_FUNCTION__; }
// P9S2D (igemm_p9s2d.h): class-uniform split-bf16 dgrad of the 3x3 stride-2 layers; JP_P9S2=0 keeps the generic DgradS2B form
inline bool p9s2_enabled() {
    static const bool on = [] { const char* e = getenv("JP_P9S2"); return !(e && e[0] == '0'); }();
    return on;
}
// per-kernel switches below JP_P9S2 (A/B and bisection): JP_P9S2D / JP_P9S2F / JP_P1S2 / JP_P7S = 0 keep the generic engine
#define JP_ENV_ON(NAME) ([] { static const bool on = [] { const char* e = getenv(NAME); return !(e && e[0] == '0'); }(); return on; }())
template <int WM, int WN, class E>
const char* p9s2d_tag() { return __PRETTY_FUNCTION__; }
template <class E>
const char* p9s2f_tag() { return __PRETTY_FUNCTION__; }
template <int CIN, class E>
const char* p7s_tag() { return __PRETTY_FUNCTION__; }
// channels per M tile of a bank with `rows` rows: 64 x (8x32 px), 128 x (4x32 px), or -- 3x3 banks whose row count is a
// multiple of 256 -- 256 x (4x32 px) on 8 waves (JP_P9_M256=0 turns that variant off)
inline bool p9_m256() {
    static const int on = [] { const char* e = getenv("JP_P9_M256"); return e ? atoi(e) : 1; }();
    return on != 0;
}
// `ptiles` = N * (H/4) * (W/32) pixel tiles of the launch (the conv entry points know it when they pack: a layer's pack is
// keyed by its shape on the host side); the 8-wave variant needs >= 256 workgroups or it leaves CUs empty
// (512->512 @32x32: 141 -> 92 TF), where it has them it is 2-4 % faster (256->256 @128x128: 141 -> 146 TF)
// (1x1 layers keep the 4x32-pixel tiles: 8x32 ones and 128-row 4-wave tiles were measured in round 4, profiles/r04_p1_tile_ab.log,
// r04_p1_tile3_ab.log; 4-wave 256-row workgroups, two per CU, in round 5: -7..-9 % alone, +0.3 ms in the step, profiles/r05_x_ab.log)
inline bool p9_wide256(int rows, long ptiles) { return p9_m256() && rows % 256 == 0 && ptiles * (rows / 256) >= 256; }
inline int p9_bmt(int rows, int khw = 9, long ptiles = 0) {
    if (rows <= 64) return 64;
    return p9_wide256(rows, ptiles) ? 256 : 128;
}
inline long p9_ptiles(int N, int H, int W) { return (long)N * (H / 4) * (W / 32); }
inline long dgrad_tap_floats(int Cin, int Cout, int KH) { return ((long)(KH * KH + 16) * Cin + 512 + 64) * ((Cout + 31) / 32 * 32); }
inline long p9_ws_floats(int rows, int red, int khw = 9) {
    const int bmt = rows <= 64 ? 64 : 128;          // the 256-row tiling of the same bank never needs more
    return ((long)jp_cdiv(red, 32) * khw * 4 + P9_QAHEAD + 1) * 8 * bmt * jp_cdiv(rows, bmt);
}
// P9S (igemm_p9s.h): the same tiles with every fp32 product formed on the bf16 matrix pipe from three-way splits of both
// operands (6 MFMAs of 32 cycles instead of 8 of 64; fp32-equivalent accuracy).  JP_P9S=0 keeps the exact-fp32 P9 kernel.
inline bool p9s_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9S"); return e ? atoi(e) : 1; }();
    return on != 0;
}
inline int p9s_kgs(int khw) { return khw == 9 ? 1 : 2; }       // 16-channel groups per stage
inline long p9s_ws_floats(int rows, int red, int khw = 9) {
    const int bmt = rows <= 64 ? 64 : 128, kgs = p9s_kgs(khw);
    return ((long)(red / (16 * kgs)) * khw * kgs + P9S_AHEAD) * (JP_NS * 8) * bmt * jp_cdiv(rows, bmt) + JP_PACK_HDR;
}
// scratch that holds either pack of a bank
inline long p9_alloc_floats(int rows, int red, int khw = 9) { return std::max(p9_ws_floats(rows, red, khw), p9s_ws_floats(rows, (red + 31) / 32 * 32, khw)); }
// fragment-order pack of a bank for the patch kernels: fp32 (PACK_FRAG) or bf16 splits (PACK_SPLIT)
inline void pack_p9(const float* w, float* wp, int Cout, int Cin, int for_dgrad, int bmt, int khw, hipStream_t st) {
    const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
    if (p9s_enabled()) do_pack(PACK_SPLIT, w, wp, p9s_ws_floats(rows, red, khw), Cout, Cin, for_dgrad, bmt, khw, p9s_kgs(khw), st);
    else do_pack(PACK_FRAG, w, wp, p9_ws_floats(rows, red, khw), Cout, Cin, for_dgrad, bmt, khw, 0, st);
}
// JP_P1: 1 = every eligible 1x1 layer, 0 = none, unset = only banks that get the 256-channel 8-wave tiles (there the
// patch kernel wins: 256->256 @256x256 forward 101 -> 107 TF, dgrad 106 -> 113 TF; with 128-channel tiles it does not)
inline int p1_mode() {
    static const int m = [] { const char* e = getenv("JP_P1"); return e ? atoi(e) : 2; }();
    return m;
}
inline bool p9_ok(int rows, int red, int N, int H, int W, int khw = 9) {
    const int tr = rows <= 64 ? 8 : 4;
    const bool p1 = p1_mode() == 1 || (p1_mode() == 2 && p9_wide256(rows, p9_ptiles(N, H, W)));
    return p9_enabled() && (khw == 9 || p1) && rows >= 32 && red >= 32 && red % (khw == 1 ? 64 : 32) == 0 && W % 32 == 0 && H % tr == 0 &&
           (long)jp_cdiv(rows, p9_bmt(rows)) * N * (H / tr) * (W / 32) >= 192;
}
template <int WM, int WN, bool REFLECT, bool REV, class E, int TAPS = 9>
const char* p9_tag() { return __PRETTY_FUNCTION__; }       // profiler tag naming the instantiation
template <int WM, int WN, bool REFLECT, bool REV, class E, int TAPS = 9>
const char* p9s_tag() { return __PRETTY_FUNCTION__; }
template <int WM, int WN, bool REFLECT, bool REV, class E, int TAPS>
const char* p9sw_tag() { return __PRETTY_FUNCTION__; }
// JP_P9_TILE (3x3 layers): 0 = 4x32-pixel tiles (rounds 2-3), 1 = 8x32-pixel wide tiles for 256-row banks, 2 = also for
// 128-row tiles (jp_igemm_p9s_wide_kernel<2, 2, ...>, 4 waves), 3 (default) = also 16x32-pixel tiles for 64-row banks (<1, 4, ...>:
// 64->64 @256^2 forward / dgrad 0.229 / 0.233 -> 0.220 / 0.209 ms).  Whole step, same box, three runs each (r04_tile_step_ab.log):
// 85.61 ms (0), 84.77 (2), 84.69 (3).
// Same box (profiles/r04_p9_tile_ab.log): 256->256 reflect @256^2 forward / dgrad 2.652 / 2.631 -> 2.513 / 2.496 ms (1 477-1 487 TF
// executed = 0.59 of 2.5 PF), @128^2 0.717 / 0.677 -> 0.678 / 0.640; 128->128 @128^2 0.197 / 0.193 -> 0.189 / 0.183.
inline int p9_tile() {
    static const int m = [] { const char* e = getenv("JP_P9_TILE"); return e ? atoi(e) : 3; }();
    return m;
}
// P1L (igemm_p1l.h, round 5): the 256-row 1x1 layers as a persistent kernel with LDS-resident weight stages -- OPT-IN (JP_P1L=1).
// Alone it is 8-9 % faster than the patch kernel on the @256^2 layers (0.556 / 0.501 -> 0.512 / 0.456 ms forward / dgrad, same pack,
// bit-identical results: profiles/r05_p1l_conv_bench.log); in the overlapped step it LOSES: same-box pairs 82.4 -> 83.2 ms with it in
// both directions, 83.2 -> 83.7 ms forward-only (profiles/r05_p1l_step_ab.log, r05_p1l_fwd_only_step_ab.log) -- a persistent workgroup
// with 144 KB of LDS and 250 registers per lane owns its CU for the whole launch, while the patch kernel's short-lived workgroups
// (49 KB, ~90 registers) let the side streams' kernels in beside them.  tests/test_kernels_gpu.py::test_p1l_persistent_1x1 runs it.
template <class E>
const char* p1l_tag() { return __PRETTY_FUNCTION__; }
inline bool p1l_enabled() {
    static const bool on = [] { const char* e = getenv("JP_P1L"); return JP_NS == 3 && e && e[0] == '1'; }();     // (written for the three-plane bf16 pack)
    return on;
}
inline int jp_num_cus() {
    static const int n = [] {
        int dev = 0, v = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        return v > 0 ? v : 256;
    }();
    return n;
}
template <bool REFLECT, bool REV, class E, int TAPS>
void launch_p9s(const float* wp, const float* x, E e, int rows, int red, int N, int H, int W, const JpCall& st, int mt_off, int bmt) {
    constexpr int KGS = TAPS == 9 ? 1 : 2;
    const int NST = red / (16 * KGS);
    // ---- the kernel and its grid, chosen ONCE: the statistics partials, the profiler tag and the launch below all follow this choice.
    // M tile bmt = 64 / 256 / 128 rows <-> WM x WN = 1x4 / 4x2 / 2x2 waves; a wave owns NJ = 2 pixel rows, 4 in the wide tiles (3x3 layers
    // only, and only where they keep every CU busy: JP_P9_TILE above)
    enum Variant { WIDE_1x4, WIDE_4x2, WIDE_2x2, NARROW_1x4, NARROW_4x2, NARROW_2x2, P1L };
    // variant = (wide or narrow block) + shape, shape = 0 / 1 / 2 for the 1x4 / 4x2 / 2x2 wave grids: both blocks list the shapes in that order
    static_assert(WIDE_4x2 == WIDE_1x4 + 1 && WIDE_2x2 == WIDE_1x4 + 2 && NARROW_4x2 == NARROW_1x4 + 1 && NARROW_2x2 == NARROW_1x4 + 2,
                  "the variant is computed as block + shape");
    const int shape = bmt == 64 ? 0 : (bmt == 256 ? 1 : 2), WN = bmt == 64 ? 4 : 2;
    const int gy = bmt == 64 ? 1 : jp_cdiv(rows, bmt == 256 ? 256 : 128);
    bool wide = false;
    if (TAPS == 9) {
        const int mode = p9_tile(), min_mode[3] = {3, 1, 2};        // least JP_P9_TILE that turns on wide tiles, by shape (1x4, 4x2, 2x2)
        wide = mode >= min_mode[shape] && H % (4 * WN) == 0 && (long)N * (H / (4 * WN)) * (W / 32) * gy >= 256;
    }
    int variant = (wide ? WIDE_1x4 : NARROW_1x4) + shape;
    dim3 grid(N * (H / ((wide ? 4 : 2) * WN)) * (W / 32), gy, 1);
    const dim3 block(bmt == 256 ? 512 : 256);
#if JP_NS == 3
    const long p1l_tiles = (long)N * (H / 4) * (W / 32), p1l_xb = (long)N * red * H * W * 4;
    const int p1l_tpw = jp_cdiv(p1l_tiles, jp_num_cus());
    if (TAPS == 1 && bmt == 256 && mt_off == 0 && p1l_enabled() && rows % 256 == 0 && red % 128 == 0 && H % 4 == 0 && W % 32 == 0 &&
        p1l_xb < (1L << 31) && p1l_tiles >= 8L * jp_num_cus()) {     // (4 tiles per workgroup, the @128^2 layers: no gain over the patch kernel, profiles/r05_p1l_conv_bench.log)
        variant = P1L;
        grid = dim3(jp_cdiv(p1l_tiles, p1l_tpw), rows / 256, 1);
    }
#endif
    const unsigned* wq = reinterpret_cast<const unsigned*>(wp);
    const float* xam = JP_NS == 2 ? jp_amax_of(x, (long)N * red * H * W, st) : nullptr;
    if constexpr (JP_NS == 2 && jp_has_amax<E>::value) e.amax = jp_take_amax_out(st);       // (every kernel below reports it)
    if constexpr (jp_has_stats<E>::value) {
        // BatchNorm statistics in the epilogue: the 4-wave 3x3 kernels only (transposed accumulators: a lane owns one channel, the
        // sums over its pixels are plain register adds + one cross-half shuffle); partials per channel = pixel tiles x pixel-row waves
        e.stats = nullptr;
        if (TAPS == 9 && bmt != 256 && mt_off == 0 && st.ax && st.ax->stats) {
            e.stats = st.ax->stats;
            st.ax->stats_parts = (int)(grid.x * WN);
        }
    }
    // executed FLOPs: JP_NPROD 16-bit MFMA products per fp32 product
    const double flops = JP_NPROD * 2.0 * rows * (double)N * H * W * TAPS * red;
    auto go = [&](const char* tag, auto kernel) {
        jp_prof_before(tag, flops, st);
        hipLaunchKernelGGL(kernel, grid, block, 0, st, wq, x, e, rows, red, NST, H, W, mt_off, xam);
        jp_prof_after(st);
    };
    switch (variant) {
        case WIDE_1x4: if constexpr (TAPS == 9) go(p9sw_tag<1, 4, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_wide_kernel<1, 4, REFLECT, REV, E, TAPS, KGS>); break;
        case WIDE_4x2: if constexpr (TAPS == 9) go(p9sw_tag<4, 2, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_wide_kernel<4, 2, REFLECT, REV, E, TAPS, KGS>); break;
        case WIDE_2x2: if constexpr (TAPS == 9) go(p9sw_tag<2, 2, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_wide_kernel<2, 2, REFLECT, REV, E, TAPS, KGS>); break;
        case NARROW_1x4: go(p9s_tag<1, 4, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_kernel<1, 4, 2, REFLECT, REV, E, TAPS, KGS>); break;
        case NARROW_4x2: go(p9s_tag<4, 2, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_kernel<4, 2, 2, REFLECT, REV, E, TAPS, KGS>); break;
        case NARROW_2x2: go(p9s_tag<2, 2, REFLECT, REV, E, TAPS>(), jp_igemm_p9s_kernel<2, 2, 2, REFLECT, REV, E, TAPS, KGS>); break;
        case P1L:
#if JP_NS == 3
            if constexpr (TAPS == 1) {
                jp_prof_before(p1l_tag<E>(), flops, st);
                hipLaunchKernelGGL((jp_conv1x1_p1l_kernel<E>), grid, block, 0, st, wq, x, e, rows, red, NST, H, W, (int)p1l_tiles, p1l_tpw, (int)p1l_xb);
                jp_prof_after(st);
            }
#endif
            break;
    }
}
// 1x1 stride-2 (ResNet downsample branches) on the same tiles: forward = P9S with a stride-2 staging gather (igemm_p9s.h, XS = 2);
// dgrad = the stride-1 kernel over the half-resolution grid with a scattering epilogue (DgradS2PointEpi)
template <int WM, int WN, class E>
const char* p9sx2_tag() { return __PRETTY_FUNCTION__; }
inline bool p1s2_ok(int rows, int red, int N, int OH, int OW) {
    const int tr = rows <= 64 ? 8 : 4;
    return p9s_enabled() && p9s2_enabled() && JP_ENV_ON("JP_P1S2") && rows >= 32 && red >= 64 && red % 64 == 0 && OW % 32 == 0 && OH % tr == 0 &&
           (long)N * red * OH * OW * 16 < (1L << 31) &&
           (long)jp_cdiv(rows, p9_bmt(rows, 1, p9_ptiles(N, OH, OW))) * N * (OH / tr) * (OW / 32) >= 192;
}
template <class E>
void launch_p1s2(const float* wp, const float* x, E e, int rows, int red, int N, int OH, int OW, const JpCall& st) {
    const int bmt = p9_bmt(rows, 1, p9_ptiles(N, OH, OW)), NST = red / 32;
    const unsigned* wq = reinterpret_cast<const unsigned*>(wp);
    const float* xam = JP_NS == 2 ? jp_amax_of(x, (long)N * red * (2L * OH) * (2L * OW), st) : nullptr;
    jp_prof_before(bmt == 64 ? p9sx2_tag<1, 4, E>() : (bmt == 256 ? p9sx2_tag<4, 2, E>() : p9sx2_tag<2, 2, E>()),
                   JP_NPROD * 2.0 * rows * (double)N * OH * OW * red, st);
    if (bmt == 64)
        hipLaunchKernelGGL((jp_igemm_p9s_x2_kernel<1, 4, 2, E>), dim3(N * (OH / 8) * (OW / 32), 1, 1), dim3(256), 0, st, wq, x, e, rows, red, NST, OH, OW, 0, xam);
    else if (bmt == 256)
        hipLaunchKernelGGL((jp_igemm_p9s_x2_kernel<4, 2, 2, E>), dim3(N * (OH / 4) * (OW / 32), jp_cdiv(rows, 256), 1), dim3(512), 0, st, wq, x, e, rows, red, NST, OH, OW, 0, xam);
    else
        hipLaunchKernelGGL((jp_igemm_p9s_x2_kernel<2, 2, 2, E>), dim3(N * (OH / 4) * (OW / 32), jp_cdiv(rows, 128), 1), dim3(256), 0, st, wq, x, e, rows, red, NST, OH, OW, 0, xam);
    jp_prof_after(st);
}
template <bool REFLECT, bool REV, class E>
void launch_p9(const float* wp, const float* x, E e, int rows, int red, int N, int H, int W, const JpCall& st, int mt_off = 0,
               int bank_rows = -1) {
    const int NCH = jp_cdiv(red, 32);
    const int bmt = p9_bmt(bank_rows < 0 ? rows : bank_rows, 9, p9_ptiles(N, H, W));   // the M tile of the PACK (the bank's rows)
    if (p9s_enabled()) { launch_p9s<REFLECT, REV, E, 9>(wp, x, e, rows, red, N, H, W, st, mt_off, bmt); return; }
    jp_prof_before(bmt == 64 ? p9_tag<1, 4, REFLECT, REV, E>() : (bmt == 256 ? p9_tag<4, 2, REFLECT, REV, E>() : p9_tag<2, 2, REFLECT, REV, E>()),
                   2.0 * rows * (double)N * H * W * 9.0 * red, st);
    if (bmt == 64) {
        dim3 grid(N * (H / 8) * (W / 32), 1, 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<1, 4, REFLECT, REV, E>), grid, dim3(256), 0, st, wp, x, e, rows, red, NCH, H, W, mt_off);
    } else if (bmt == 256) {
        dim3 grid(N * (H / 4) * (W / 32), jp_cdiv(rows, 256), 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<4, 2, REFLECT, REV, E>), grid, dim3(512), 0, st, wp, x, e, rows, red, NCH, H, W, mt_off);
    } else {
        dim3 grid(N * (H / 4) * (W / 32), jp_cdiv(rows, 128), 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<2, 2, REFLECT, REV, E>), grid, dim3(256), 0, st, wp, x, e, rows, red, NCH, H, W, mt_off);
    }
    jp_prof_after(st);
}
// 1x1 stride-1 convolution / its dgrad through the same kernel (TAPS = 1, two channel chunks per stage)
template <class E>
void launch_p1(const float* wp, const float* x, E e, int rows, int red, int N, int H, int W, const JpCall& st) {
    const int NST = jp_cdiv(red, 64);
    const int bmt = p9_bmt(rows, 1, p9_ptiles(N, H, W));
    if (p9s_enabled()) { launch_p9s<false, false, E, 1>(wp, x, e, rows, red, N, H, W, st, 0, bmt); return; }
    jp_prof_before(bmt == 64 ? p9_tag<1, 4, false, false, E, 1>() : (bmt == 256 ? p9_tag<4, 2, false, false, E, 1>() : p9_tag<2, 2, false, false, E, 1>()),
                   2.0 * rows * (double)N * H * W * red, st);
    if (bmt == 64) {
        dim3 grid(N * (H / 8) * (W / 32), 1, 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<1, 4, false, false, E, 1, 2>), grid, dim3(256), 0, st, wp, x, e, rows, red, NST, H, W, 0);
    } else if (bmt == 256) {
        dim3 grid(N * (H / 4) * (W / 32), rows / 256, 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<4, 2, false, false, E, 1, 2>), grid, dim3(512), 0, st, wp, x, e, rows, red, NST, H, W, 0);
    } else {
        dim3 grid(N * (H / 4) * (W / 32), jp_cdiv(rows, 128), 1);
        hipLaunchKernelGGL((jp_igemm_p9_kernel<2, 2, false, false, E, 1, 2>), grid, dim3(256), 0, st, wp, x, e, rows, red, NST, H, W, 0);
    }
    jp_prof_after(st);
}

// split-K factor for forward / dgrad launches whose tile grid cannot fill 256 CUs (pose encoder, 32x32 .. 6x20 maps)
inline int small_grid_splits(int M, long N, int Kp) {
    const int bm = M <= 64 ? 64 : (N <= 64 ? 256 : 128), bn = M <= 64 ? 256 : (N <= 64 ? 64 : 128);
    const long tiles = (long)jp_cdiv(M, bm) * jp_cdiv(N, bn);
    if (tiles >= 192) return 1;
    const int chunks = Kp / KC;
    int sp = (int)std::min<long>(jp_cdiv(512, tiles), chunks / 8);
    return std::max(1, sp);
}
inline bool seg_aligned(int c0, int c1, int c2) {   // every segment end except the last is a multiple of 32
    if (c1 == 0 && c2 == 0) return true;
    if (c0 % 32) return false;
    if (c2 != 0 && (c0 + c1) % 32) return false;
    return true;
}

}  // namespace

extern "C" int jp_conv2d_up_head_ok(int c0, int up0, int c1, int c2, int Cout, int KH, int stride, int pad, int pad_mode, int H,
                                    int W) {
    return up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W) ? 1 : 0;
}
// floats of caller-owned scratch for the packed-weight fast path (0 = the generic path will be used).
// which: 0 forward, 1 dgrad, 2 wgrad
// does the small-map split-bf16 path (conv_p9sm.hip) take this stride-1 3x3 / 1x1 GEMM (rows x red over N x H x W pixels)?
// JP_P9SM = 2 (default): every eligible layer the regular patch kernels do not run (also the 1x1 layers with 64 / 128-row
// banks, which those leave to the generic engine: reduce 128->256 @128^2 dgrad 0.116 -> 0.066 ms, 64->256 @256^2 0.217 -> 0.187);
// 1: only what they reject for their tile shape or grid size (maps that are not multiples of the pixel tile, < 192 workgroups);
// 0: off.
static bool p9sm_wanted(int rows, int red, int N, int H, int W, int KH, int stride, int pad, JpP9smPlan* sm) {
    static const int mode = [] { const char* e = getenv("JP_P9SM"); return e ? atoi(e) : 2; }();
    if (!mode || stride != 1 || !((KH == 3 && pad == 1) || (KH == 1 && pad == 0))) return false;
    if (p9_ok(rows, red, N, H, W, KH * KH)) return false;
    if (!jp_p9sm_plan(rows, red, N, H, W, KH * KH, sm)) return false;
    const bool odd_shape = W % 32 != 0 || H % sm->tr != 0;
    return mode >= 2 || odd_shape || sm->splits > 1 ||
           (long)jp_cdiv(rows, sm->bmt) * N * jp_cdiv(H, sm->tr) * jp_cdiv(W, 32) < 192;
}

// floats of `bn_stats` scratch for a forward call with OH x OW output maps: 2 sums x Cout x (at most one partial per 2 x 32 output pixels)
extern "C" long jp_conv2d_fwd_bn_stats_floats(int N, int OH, int OW, int Cout) {
    return 2L * Cout * N * jp_cdiv(OH, 2) * jp_cdiv(OW, 32);
}
extern "C" long jp_conv2d_ws_floats(int Cin, int Cout, int KH, int which) {
    // + 256 rows of slack: the A gather of the last M tile reads (never uses) up to 255 rows past the last tap
    // forward: up to 16 weight planes per channel (parity-class path of fused-upsample segments), 3 padded segments
    if (which == 0 && Cin <= 8) return (long)(Cout + 256) * pad32(KH * KH * 8);   // row-major pack of the stem path
    if (which == 0) return Cin >= 16 ? std::max(std::max(((long)std::max(KH * KH, 16) * Cout + 256) * (pad32(Cin) + 96),
                                                         // P9US pack: <= 16 steps per 16 channels (4 classes x 4 slots) + D + slack
                                                         KH == 3 ? (long)jp_cdiv(Cout, 128) * ((long)jp_cdiv(Cin, 16) * 16 + 10) * 3072 : 0L),
                                                KH == 3 ? p9_alloc_floats(Cout, pad32(Cin)) : (KH == 1 ? p9_alloc_floats(Cout, pad32(Cin), 1) : 0L)) : 0;
    // dgrad: [tap][ci][Cp] + slack, plus 16 planes [class,slot][c][Cp] + slack for jp_conv2d_dgrad_src3's upsampled
    // segment, plus the fragment-order pack of the P9 main pass behind them
    if (which == 1) return Cout >= 16 ? dgrad_tap_floats(Cin, Cout, KH) + (KH == 3 ? p9_alloc_floats(Cin, pad32(Cout)) + p9sd_floats(Cin, Cout) : (KH == 1 ? p9_alloc_floats(Cin, pad32(Cout), 1) : 0L)) : 0;
    return 0;
}

extern "C" int jp_conv2d_fwd_src3(const float* x0, int c0, int up0, const float* x1, int c1, int up1,
                                  const float* x2, int c2, int up2, const float* w, const float* bias, float* y,
                                  int N, int H, int W, int Cout, int KH, int stride, int pad, int pad_mode, int act,
                                  float* ws, int ws_state, float* split_ws, const float* amax_x0, const float* amax_x1,
                                  const float* amax_x2, float* amax_y, int* amax_y_done, float* amax_ws, float* bn_stats,
                                  int* bn_stats_parts, void* stream) {
    // ws_state: 0 = pack the weights into ws now; 1 = ws already holds this layer's pack (refreshed by jp_pack_replay)
    // amax_*: operand magnitudes of the fp16 split kernels, see the header (all may be NULL when amax_ws is given)
    // bn_stats: optional scratch of jp_conv2d_fwd_bn_stats_floats floats for a convolution that feeds a train-mode BatchNorm (no bias, no
    // activation): the 4-wave 3x3 patch kernels leave per-channel partial sums of y and y^2 there and *bn_stats_parts (host int) = the
    // partials per channel, to be handed to jp_bn_train_fwd instead of its own pass over y; 0 = the kernel that ran does not (BatchNorm
    // then reads y itself, as before)
    if (amax_y_done) *amax_y_done = 0;
    if (bn_stats_parts) *bn_stats_parts = 0;
    JP_CHECK_ARG(x0 && w && y, "conv2d_fwd: null pointer");
    JP_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cout > 0 && c0 > 0 && stride >= 1, "conv2d_fwd: bad dims");
    JP_CHECK_ARG(!(pad_mode == JP_PAD_REFLECT && (pad >= H || pad >= W)), "conv2d_fwd: reflect pad >= size");
    const int Cin = c0 + c1 + c2;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const long npix = (long)N * OH * OW;
    JP_CHECK_ARG(npix < (1L << 31) && (long)N * Cin * H * W < (1L << 31) * 2, "conv2d_fwd: tensor too large");
    // (a multi-source call always needs the scratch: the kernel reads ONE magnitude, the largest of the sources', folded into amax_ws)
    JP_CHECK_ARG(JP_NS != 2 || amax_ws || (amax_x0 && !c1 && !c2),
                 "conv2d_fwd"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(x0, amax_x0);
    ax.know(x1, amax_x1);
    ax.know(x2, amax_x2);
    ax.ws = amax_ws;
    ax.out = reinterpret_cast<unsigned*>(amax_y);
    if (bn_stats && bn_stats_parts && !bias && act == JP_ACT_NONE) ax.stats = bn_stats;
    const JpAmaxDone done_flag{amax_y_done, &ax, bn_stats_parts};
    const JpCall st((hipStream_t)stream, &ax);
    FwdEpi e{y, bias, Cout, OH * OW, act};
    if (up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W)) {
        jp_up_head_fwd(x0, w, bias, y, N, c0, H / 2, W / 2, act, st);
        JP_LAUNCH_CHECK();
    }
    if (small_head(Cin, Cout, KH, stride, pad)) {
        jp_conv_small_fwd(x0, c0, up0, x1, c1, up1, x2, c2, up2, w, bias, y, N, H, W, Cout, act,
                          pad_mode == JP_PAD_REFLECT, st);
        JP_LAUNCH_CHECK();
    }
    if (c1 == 0 && c2 == 0 && jp_c16_ok(c0, Cout, KH, stride, pad, pad_mode, H, W)) {
        jp_c16_fwd(x0, up0, w, bias, y, N, c0, Cout, H, W, act, st);
        JP_LAUNCH_CHECK();
    }
    const Src3 src = make_src(x0, c0, up0, x1, c1, up1, x2, c2, up2, H, W);
    if (ws && Cin <= 8 && Cout <= 64 && c1 == 0 && c2 == 0 && !up0 && pad_mode != JP_PAD_REFLECT && (KH == 7 || KH == 3) &&
        npix / 256 >= 192 && (long)2 * Cin * H * W * 4 < (1L << 32)) {
        if (KH == 7 && stride == 2 && pad == 3 && (Cin == 3 || Cin == 6) && p9s_enabled() && p9s2_enabled() && JP_ENV_ON("JP_P7S") && H == 2 * OH && W == 2 * OW &&
            OH % 8 == 0 && OW % 32 == 0 && (long)Cin * H * W * 4 < (1L << 31)) {
            // P7S stem kernel (igemm_p7s.h): split-bf16 products, the whole K of a tile staged once
            const long tot = (4L * Cin + 1) * (JP_NS * 512) + JP_PACK_HDR;
            if (!ws_state) do_pack(PACK_SPLIT7, w, ws, tot, Cout, Cin, 0, 0, 0, 0, st);
            const int ntiles = N * (OH / 8) * (OW / 32);
            const unsigned* wq = reinterpret_cast<const unsigned*>(ws);
            const float* xam = JP_NS == 2 ? jp_amax_of(x0, (long)N * Cin * H * W, st) : nullptr;
            jp_prof_before(Cin == 3 ? p7s_tag<3, FwdEpi>() : p7s_tag<6, FwdEpi>(), JP_NPROD * 2.0 * 64 * (double)npix * 64.0 * Cin, st);
            if (Cin == 3) hipLaunchKernelGGL((jp_igemm_p7s_kernel<3, FwdEpi>), dim3(ntiles), dim3(256), 0, st, wq, x0, e, Cout, OH, OW, ntiles, xam);
            else hipLaunchKernelGGL((jp_igemm_p7s_kernel<6, FwdEpi>), dim3(ntiles), dim3(256), 0, st, wq, x0, e, Cout, OH, OW, ntiles, xam);
            jp_prof_after(st);
            JP_LAUNCH_CHECK();
        }
        // stem convs: whole taps per K chunk
        const int CP = Cin <= 4 ? 4 : 8;
        const int Kp = jp_cdiv(KH * KH * CP, KC) * KC;
        if (!ws_state) do_pack(PACK_ROWMAJOR, w, ws, (long)Cout * Kp, Cout, Cin, KH * KH, CP, Kp, 0, st);
        PackARow a{ws, Kp};
#define JP_BC(KHv, CPv)                                                          \
    {                                                                            \
        FwdBC<KHv, CPv> b{x0, Cin, H, W, (int)npix, OH, OW, stride, pad};        \
        launch<false, 1, 4>(a, b, e, Cout, (int)npix, Kp, 1, Kp, st);            \
    }
        if (KH == 7 && CP == 4) JP_BC(7, 4)
        else if (KH == 7) JP_BC(7, 8)
        else if (CP == 4) JP_BC(3, 4)
        else JP_BC(3, 8)
#undef JP_BC
        JP_LAUNCH_CHECK();
    }
    // P9U patch kernel for the iconv layers: cat(skip (full res), up2x(x), disparity channel) -> Cout, reflection pad
    if (ws && p9_enabled() && KH == 3 && stride == 1 && pad == 1 && pad_mode == JP_PAD_REFLECT && c0 >= 32 && c0 % 32 == 0 &&
        !up0 && c1 >= 32 && c1 % 32 == 0 && up1 && c2 <= 8 && !(c2 && up2) && Cout % 128 == 0 && H % 4 == 0 && W % 64 == 0 &&
        (long)(Cout / 128) * N * (H / 4) * (W / 64) >= 128 && p9u_enabled()) {
        const int MT = Cout / 128;
        if (p9us_enabled()) {
            // P9US2: the same tiles on the bf16 matrix pipe (three-way split products, igemm_p9us2.h)
            constexpr long SF = JP_NS * 1024;         // floats per weight step
            const long fS = (long)MT * (c0 / 16) * 9 * SF, fU = 4L * MT * (c1 / 16) * 4 * SF, fD = c2 ? (long)MT * 9 * SF : 0;
            constexpr int HD = JP_PACK_HDR;           // one scale header in front of the bank (JP_NS == 2); every segment knows how far back
            if (!ws_state) {
                do_pack(PACK_SPLITSEG, w, ws + HD, fS, Cout, Cin, 0, c0, 0, HD, st);
                do_pack(PACK_SPLITSEG, w, ws + HD + fS, fU, Cout, Cin, c0, c1, 1, (int)(HD + fS), st);
                if (c2) do_pack(PACK_SPLITSEG, w, ws + HD + fS + fU, fD, Cout, Cin, c0 + c1, c2, 0, (int)(HD + fS + fU), st);
                // (the kernel's last weight prefetch reads one step past the streams: inside the scratch, never used)
            }
            // P9US2 (igemm_p9us2.h, round 5): every operand request inside an MFMA pair's shadow, the next patch staged by the half of
            // the workgroup that is off the pipe.  (The round-3 stream, its 8-row tiles and its double buffer are gone: logs in
            // profiles/r04_p9us_*.log, r05_p9us2_*.log.)
            const float* xam = JP_NS == 2 ? jp_amax_of3(x0, (long)N * c0 * H * W, x1, (long)N * c1 * (H / 2) * (W / 2), x2,
                                                        c2 ? (long)N * c2 * H * W : 0L, st) : nullptr;
            e.amax = jp_take_amax_out(st);
            jp_prof_before(p9us2_tag<FwdEpi>(), JP_NPROD * 2.0 * Cout * (double)npix * (9.0 * c0 + 4.0 * c1 + 9.0 * (c2 ? 16 : 0)), st);
            hipLaunchKernelGGL((jp_igemm_p9us2_kernel<FwdEpi>), dim3(N * (H / 4) * (W / 64), MT, 1), dim3(512), 0, st,
                               reinterpret_cast<const unsigned*>(ws), x0, x1, x2, e, Cout, c0, c1, c2, H, W, xam);
            jp_prof_after(st);
            JP_LAUNCH_CHECK();
        }
        const long fS = (long)MT * (c0 / 32) * 36 * 1024, fU = 4L * MT * (c1 / 32) * 16 * 1024, fD = (long)MT * 9 * 1024;
        if (!ws_state) {
            do_pack(PACK_FRAGSEG, w, ws, fS, Cout, Cin, 0, c0, 16, 0, st);
            do_pack(PACK_FRAGSEG, w, ws + fS, fU, Cout, Cin, c0, c1, 16, 1, st);
            if (c2) do_pack(PACK_FRAGSEG, w, ws + fS + fU, fD, Cout, Cin, c0 + c1, c2, 4, 0, st);
        }
        jp_prof_before(p9u_tag<FwdEpi>(), 2.0 * Cout * (double)npix * (9.0 * c0 + 4.0 * c1 + 9.0 * c2), st);
        dim3 grid(N * (H / 4) * (W / 64), MT, 1);
        hipLaunchKernelGGL((jp_igemm_p9u_kernel<FwdEpi>), grid, dim3(512), 0, st, ws, x0, x1, x2, e, Cout, c0, c1, c2, H, W);
        jp_prof_after(st);
        JP_LAUNCH_CHECK();
    }
    const bool any_up = (c0 && up0) || (c1 && up1) || (c2 && up2);
    {   // upsample-aware parity-class path (iconv layers)
        const long Ncl = (long)N * (H / 2) * (W / 2);
        if (ws && any_up && KH == 3 && stride == 1 && pad == 1 && pad_mode == JP_PAD_REFLECT && H % 2 == 0 && W % 2 == 0 &&
            Ncl % 256 == 0 && seg_aligned(c0, c1, c2) && Cin >= 32 && (long)jp_cdiv(Cout, 128) * (npix / 128) >= 192) {
            const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2};
            int T[3], P[3], O[3], nch[3];
            long off = 0;
            for (int i = 0; i < 3; ++i) {
                T[i] = us[i] ? 4 : 9;
                P[i] = pad32(cs[i]);
                nch[i] = P[i] / 32;
                O[i] = (int)off;
                if (cs[i]) {
                    const long tot = (long)(us[i] ? 16 : 9) * Cout * P[i];
                    if (!ws_state) do_pack(PACK_SEG, w, ws + off, tot, Cout, Cin, (i == 0 ? 0 : (i == 1 ? c0 : c0 + c1)), cs[i], P[i], us[i], st);
                    off += tot;
                }
            }
            ParSeg ps{nch[0] * T[0], nch[0] * T[0] + nch[1] * T[1], T[0], T[1], T[2], O[0], O[1], O[2], P[0], P[1], P[2]};
            const int Q = ps.q1 + nch[2] * T[2];
            PackAP a{ws, ps, Cout, (int)Ncl};
            FwdBP b{src, ps, (int)Ncl, H / 2, W / 2};
            FwdEpiP ep{y, bias, Cout, (int)Ncl, H / 2, W / 2, act};
            launch_auto(a, b, ep, Cout, (int)npix, Q * KC, 1, Q * KC, st);
            JP_LAUNCH_CHECK();
        }
    }
    if (ws && Cin >= 16 && seg_aligned(c0, c1, c2)) {   // tap-major fast path (16-channel inputs: half-empty K chunks)
        const int Cp = pad32(Cin), Kp = KH * KH * Cp;
        const bool use_p9 = KH == 3 && stride == 1 && pad == 1 && !any_up && c1 == 0 && c2 == 0 && p9_ok(Cout, Cin, N, H, W);
        const bool use_p1 = KH == 1 && stride == 1 && pad == 0 && !any_up && c1 == 0 && c2 == 0 && p9_ok(Cout, Cin, N, H, W, 1);
        if (KH == 1 && stride == 2 && pad == 0 && c1 == 0 && c2 == 0 && !up0 && H % 2 == 0 && W % 2 == 0 &&
            p1s2_ok(Cout, Cin, N, OH, OW)) {
            if (!ws_state) pack_p9(w, ws, Cout, Cin, 0, p9_bmt(Cout, 1, p9_ptiles(N, OH, OW)), 1, st);
            launch_p1s2(ws, x0, e, Cout, Cin, N, OH, OW, st);
            JP_LAUNCH_CHECK();
        }
        if (use_p1) {      // 1x1: weights stream in fragment order, two channel chunks of the pixel tile staged per barrier pair
            if (!ws_state) pack_p9(w, ws, Cout, Cin, 0, p9_bmt(Cout, 1, p9_ptiles(N, H, W)), 1, st);
            launch_p1(ws, x0, e, Cout, Cin, N, H, W, st);
            JP_LAUNCH_CHECK();
        }
        if (KH == 3 && stride == 2 && pad == 1 && pad_mode != JP_PAD_REFLECT && c1 == 0 && c2 == 0 && !up0 && p9s_enabled() &&
            p9s2_enabled() && JP_ENV_ON("JP_P9S2F") && H == 2 * OH && W == 2 * OW && OH % 4 == 0 && OW % 32 == 0 && Cin % 16 == 0 && Cin >= 32 && Cout > 64 &&
            (long)N * Cin * H * W * 4 < (1L << 31) && (long)jp_cdiv(Cout, 128) * N * (OH / 4) * (OW / 32) >= 192) {
            // 3x3 stride 2: P9S2F patch kernel (igemm_p9s2f.h) on the P9S forward pack (instead of the tap-major one)
            if (!ws_state) pack_p9(w, ws, Cout, Cin, 0, 128, 9, st);
            const float* xam = JP_NS == 2 ? jp_amax_of(x0, (long)N * Cin * H * W, st) : nullptr;
            jp_prof_before(p9s2f_tag<FwdEpi>(), JP_NPROD * 2.0 * Cout * (double)npix * 9.0 * Cin, st);
            hipLaunchKernelGGL((jp_igemm_p9s2f_kernel<FwdEpi>), dim3(N * (OH / 4) * (OW / 32), jp_cdiv(Cout, 128), 1), dim3(256), 0, st,
                               reinterpret_cast<const unsigned*>(ws), x0, e, Cout, Cin, Cin / 16, OH, OW, xam);
            jp_prof_after(st);
            JP_LAUNCH_CHECK();
        }
        if (use_p9) {
            // P9 patch kernel: the input patch of a 4x32 pixel tile is staged once per channel chunk for all 9 taps,
            // weights stream from L2 in MFMA fragment order (igemm_p9.h); its pack takes the place of the tap-major one
            if (!ws_state) pack_p9(w, ws, Cout, Cin, 0, p9_bmt(Cout, 9, p9_ptiles(N, H, W)), 9, st);
            if (pad_mode == JP_PAD_REFLECT) launch_p9<true, false>(ws, x0, e, Cout, Cin, N, H, W, st);
            else launch_p9<false, false>(ws, x0, e, Cout, Cin, N, H, W, st);
            JP_LAUNCH_CHECK();
        }
        {   // small maps (partial tiles, split-K over the channel stages) on the split-bf16 patch kernel (conv_p9sm.hip)
            JpP9smPlan sm;
            if (c1 == 0 && c2 == 0 && !up0 && p9sm_wanted(Cout, Cin, N, H, W, KH, stride, pad, &sm) && (sm.splits == 1 || split_ws)) {
                if (!ws_state) pack_p9(w, ws, Cout, Cin, 0, sm.bmt, KH * KH, st);
                jp_p9sm_launch(sm, ws, x0, y, bias, act, 0, split_ws, Cout, Cin, N, H, W, KH * KH, pad_mode == JP_PAD_REFLECT, 0, st);
                if (sm.splits > 1) slice_reduce_nchw(split_ws, y, bias, Cout, (int)npix, OH * OW, sm.splits, act, 0, st);
                JP_LAUNCH_CHECK();
            }
        }
        if (!ws_state) pack_weights(w, ws, Cout, Cin, KH * KH, Cp, 0, st);
        PackA a{ws, Cout, Kp, Cp, KH * KH};
        // the tap-major launch over `splits` K slices of kps elements, for either pad mode, into epilogue ep
        auto launch_taps = [&](auto ep, int splits, int kps) -> int {
            JP_KH_SWITCH(KH, {
                if (pad_mode == JP_PAD_REFLECT) {
                    FwdBT<KH_, true> b{src, Cp, (int)npix, OH, OW, stride, pad};
                    launch_auto(a, b, ep, Cout, (int)npix, Kp, splits, kps, st);
                } else {
                    FwdBT<KH_, false> b{src, Cp, (int)npix, OH, OW, stride, pad};
                    launch_auto(a, b, ep, Cout, (int)npix, Kp, splits, kps, st);
                }
            });
            return JP_OK;
        };
        const int sp = small_grid_splits(Cout, npix, Kp);
        if (sp > 1) {
            const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
            if (split_ws) {   // per-slice partial tiles + fixed-order reduction: bit-reproducible forward
                WgradEpiWS es{split_ws, Cout, (int)npix};
                if (const int rc = launch_taps(es, jp_cdiv(Kp, kps), kps)) return rc;
                slice_reduce_nchw(split_ws, y, bias, Cout, (int)npix, OH * OW, jp_cdiv(Kp, kps), act, 0, st);
                JP_LAUNCH_CHECK();
            }
            JP_HIP(hipMemsetAsync(y, 0, sizeof(float) * (size_t)npix * Cout, st));
            AtomicEpi ea{y, Cout, OH * OW};
            if (const int rc = launch_taps(ea, jp_cdiv(Kp, kps), kps)) return rc;
            if (bias || act != JP_ACT_NONE) {
                const long total = npix * Cout;
                hipLaunchKernelGGL(bias_act_nchw_kernel, dim3((int)std::min<long>((total + 255) / 256, 2048)), dim3(256), 0, st,
                                   y, bias, total, Cout, OH * OW, act);
            }
            JP_LAUNCH_CHECK();
        }
        const int bn3 = Cout <= 64 ? 256 : 128;
        if (KH == 3 && stride == 1 && pad == 1 && !any_up && Cin >= 32 && W % bn3 == 0 && npix > 64) {
            // row-tile kernel: the three dx taps share one staged input row segment
            if (pad_mode == JP_PAD_REFLECT) {
                if (Cout <= 64) { FwdBR3<true, false, 256> b{src, H, W}; launch_r3<1, 4>(a, b, e, Cout, (int)npix, Kp, st); }
                else { FwdBR3<true, false, 128> b{src, H, W}; launch_r3<2, 2>(a, b, e, Cout, (int)npix, Kp, st); }
            } else {
                if (Cout <= 64) { FwdBR3<false, false, 256> b{src, H, W}; launch_r3<1, 4>(a, b, e, Cout, (int)npix, Kp, st); }
                else { FwdBR3<false, false, 128> b{src, H, W}; launch_r3<2, 2>(a, b, e, Cout, (int)npix, Kp, st); }
            }
            JP_LAUNCH_CHECK();
        }
        if (const int rc = launch_taps(e, 1, Kp)) return rc;
    } else {
        const int K = Cin * KH * KH;
        FwdA a{w, Cout, K};
        JP_KH_SWITCH(KH, {
            FwdB<KH_> b{src, K, (int)npix, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
            launch_auto(a, b, e, Cout, (int)npix, K, 1, jp_cdiv(K, KC) * KC, st);
        });
    }
    JP_LAUNCH_CHECK();
}

extern "C" int jp_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H,
                             int W, int Cout, int KH, int stride, int pad, int pad_mode, int act, float* ws,
                             int ws_state, float* split_ws, const float* amax_x, float* amax_y, int* amax_y_done, float* amax_ws,
                             float* bn_stats, int* bn_stats_parts, void* stream) {
    return jp_conv2d_fwd_src3(x, Cin, 0, nullptr, 0, 0, nullptr, 0, 0, w, bias, y, N, H, W, Cout, KH, stride, pad,
                              pad_mode, act, ws, ws_state, split_ws, amax_x, nullptr, nullptr, amax_y, amax_y_done, amax_ws, bn_stats,
                              bn_stats_parts, stream);
}

// same for jp_conv2d_dgrad's `split_ws`
extern "C" long jp_conv2d_dgrad_split_floats(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad) {
    if (Cout < 16) return 0;
    const long npix = (long)N * H * W;
    const int Kp = KH * KH * pad32(Cout);
    // 3x3 stride 2: the parity-class forms need no split; maps they do not take (N * H/2 * W/2 not a multiple of 256: the 8 x 8 maps of
    // the 256^2 test shapes) run the generic loader, whose small-grid K slices must not meet in atomics (round 6: that was the first
    // run-dependent sum of the backward at those shapes, tools/debug/first_divergence.py)
    if (KH == 3 && stride == 2 && pad == 1 && H % 2 == 0 && W % 2 == 0 && ((long)N * (H / 2) * (W / 2)) % 256 == 0) return 0;
    // reflection layers (the pad mode is not an argument here: every 3x3 stride-1 pad-1 layer gets it): <= 4 slices of the
    // border pass, part[slice][Cin][N * (2H + 2W)]
    long border = (KH == 3 && stride == 1 && pad == 1) ? 4L * Cin * N * (2L * H + 2L * W) : 0;
    JpP9smPlan sm;
    if (p9sm_wanted(Cin, Cout, N, H, W, KH, stride, pad, &sm)) border = std::max(border, sm.part_floats);
    const int sp = small_grid_splits(Cin, npix, Kp);
    if (sp <= 1) return border;
    const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
    return std::max(border, (long)jp_cdiv(Kp, kps) * Cin * npix);
}

// floats of optional caller scratch (`split_ws`) for the split-K forward of layers whose tile grid cannot fill the
// chip: with it the K slices are reduced in a fixed order (bit-reproducible); without it they meet in atomics.
extern "C" long jp_conv2d_fwd_split_floats(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad) {
    if (Cin < 16) return 0;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const long npix = (long)N * OH * OW;
    const int Kp = KH * KH * pad32(Cin);
    JpP9smPlan sm;
    const long smf = p9sm_wanted(Cout, Cin, N, H, W, KH, stride, pad, &sm) ? sm.part_floats : 0;
    const int sp = small_grid_splits(Cout, npix, Kp);
    if (sp <= 1) return smf;
    const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
    return std::max(smf, (long)jp_cdiv(Kp, kps) * Cout * npix);
}

// reflection border pass of a dgrad (rows of `a` = the C input channels of this call): through caller scratch when there is some
// (K slices stored coalesced, one fixed-order fold into dx), else the read-modify-write epilogue
static void border_pass(const PackA& a, const float* dy, float* dx, int C, int Cp, int Kp, int Cout, int N, int H, int W,
                        float* split_ws, const JpCall& st) {
    const int Nb = N * (2 * W + 2 * H);
    DgradBorderB<3> bb{dy, Cp, Nb, H, W, Cout};
    const long btiles = (long)jp_cdiv(C, C <= 64 ? 64 : 128) * jp_cdiv(Nb, C <= 64 ? 256 : 128);
    static const bool via_ws = [] { const char* e_ = getenv("JP_BORDER_WS"); return !(e_ && e_[0] == '0'); }();
    const int chunks = Kp / KC;
    const int wsl = (int)std::max<long>(1, std::min<long>(std::min<long>(4, chunks / 9), jp_cdiv(512, btiles)));
    if (via_ws && split_ws && wsl > 1) {      // (also the one-row launches -- the disparity channel: its slices met in float atomics until round 6)
        const int wkps = jp_cdiv(jp_cdiv(Kp, wsl), KC) * KC, nsl = jp_cdiv(Kp, wkps);
        WgradEpiWS es{split_ws, C, Nb};
        launch_auto(a, bb, es, C, Nb, Kp, nsl, wkps, st);
        const long total = (long)C * Nb;
        hipLaunchKernelGGL(border_add_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, split_ws, dx, C, Nb, H,
                           W, nsl, (st.ax && st.ax->out_taken) ? st.ax->out : nullptr);
        return;
    }
    if (st.ax) st.ax->out_taken = false;       // (the read-modify-write epilogue below does not report: the caller reduces dx itself)
    DgradBorderEpi be{dx, C, H, W, Nb, 0};
    const int bsp = border_splits(btiles, Kp / KC);
    const int bkps = jp_cdiv(jp_cdiv(Kp, bsp), KC) * KC;
    be.split = jp_cdiv(Kp, bkps) > 1;
    launch_auto(a, bb, be, C, Nb, Kp, jp_cdiv(Kp, bkps), bkps, st);
}

// rows of a short row tail, 0 = none: 513 = 4*128 + 1 input channels of the iconv layers run the tail as its own 64-row launch
// instead of a fifth, almost empty 128-row tile column
static inline int dgrad_row_tail(int Cin) { return (Cin > 128 && Cin % 128 <= 16) ? Cin % 128 : 0; }

extern "C" int jp_conv2d_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int H, int W, int Cout,
                               int KH, int stride, int pad, int pad_mode, int accumulate, float* ws, int ws_state,
                               float* split_ws, const float* amax_dy, float* amax_dx, int* amax_dx_done, float* amax_ws,
                               void* stream) {
    if (amax_dx_done) *amax_dx_done = 0;
    JP_CHECK_ARG(dy && w && dx, "conv2d_dgrad: null pointer");
    JP_CHECK_ARG(!(pad_mode == JP_PAD_REFLECT && !(KH == 3 && stride == 1 && pad == 1 && H >= 2 && W >= 2)),
                 "conv2d_dgrad: reflect mode supports 3x3 stride 1 pad 1 only");
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const long npix = (long)N * H * W;
    JP_CHECK_ARG(npix < (1L << 31), "conv2d_dgrad: tensor too large");
    JP_CHECK_ARG(JP_NS != 2 || amax_ws || amax_dy, "conv2d_dgrad"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(dy, amax_dy);
    ax.ws = amax_ws;
    // amax_dx: folded in by the patch kernels' epilogue (+ the border fold of reflection layers); a layer with a short row tail is
    // finished by a second launch that does not report, so the slot is not offered there
    if (!dgrad_row_tail(Cin)) ax.out = reinterpret_cast<unsigned*>(amax_dx);
    const JpAmaxDone done_flag{amax_dx_done, &ax};
    const JpCall st((hipStream_t)stream, &ax);
    if (jp_c16_ok(Cin, Cout, KH, stride, pad, pad_mode, H, W)) {
        jp_c16_dgrad(dy, w, dx, 0, N, Cin, Cout, H, W, accumulate, st);
        JP_LAUNCH_CHECK();
    }
    DgradEpi e{dx, Cin, H * W, accumulate};
    if (ws && Cout >= 16) {
        const int Cp = pad32(Cout), Kp = KH * KH * Cp;
        const int sp = small_grid_splits(Cin, npix, Kp);
        // zero-padded 3x3 stride-1 layers that the P9 main pass covers completely (no row tail, no reflection border pass)
        // never read the tap-major pack: it is neither built nor replayed for them
        const bool p9_only = KH == 3 && stride == 1 && pad == 1 && pad_mode != JP_PAD_REFLECT && sp <= 1 &&
                             !dgrad_row_tail(Cin) && p9_ok(Cin, Cout, N, H, W);
        const long Nc = (long)N * (H / 2) * (W / 2);
        // 3x3 stride-2 layers: class-uniform split-bf16 kernel on the half-resolution grid (its own fragment-order pack only)
        const bool s2_form = KH == 3 && stride == 2 && pad == 1 && pad_mode != JP_PAD_REFLECT && H % 2 == 0 && W % 2 == 0 &&
                             2 * OH == H && 2 * OW == W;
        if (s2_form && p9s_enabled() && p9s2_enabled() && JP_ENV_ON("JP_P9S2D") && Cin >= 32 && Cout % 16 == 0 && OW % 32 == 0 &&
            OH % (Cin <= 64 ? 8 : 4) == 0 && (long)N * Cout * OH * OW * 4 < (1L << 31) &&
            (long)jp_cdiv(Cin, Cin <= 64 ? 64 : 128) * N * (OH / (Cin <= 64 ? 8 : 4)) * (OW / 32) * 4 >= 192) {
            float* wfr = ws + dgrad_tap_floats(Cin, Cout, KH);
            const int bmt = Cin <= 64 ? 64 : 128;
            if (!ws_state) pack_p9(w, wfr, Cout, Cin, 1, bmt, 9, st);
            const unsigned* wq = reinterpret_cast<const unsigned*>(wfr);
            const int NST = Cout / 16;
            const float* xam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * OH * OW, st) : nullptr;
            jp_prof_before(bmt == 64 ? p9s2d_tag<1, 4, DgradEpi>() : p9s2d_tag<2, 2, DgradEpi>(),
                           JP_NPROD * 2.0 * Cin * (double)N * OH * OW * 9.0 * Cout, st);
            if (bmt == 64)
                hipLaunchKernelGGL((jp_igemm_p9s2d_kernel<1, 4, 2, DgradEpi>), dim3(4 * N * (OH / 8) * (OW / 32), 1, 1), dim3(256), 0, st,
                                   wq, dy, e, Cin, Cout, NST, OH, OW, xam);
            else
                hipLaunchKernelGGL((jp_igemm_p9s2d_kernel<2, 2, 2, DgradEpi>), dim3(4 * N * (OH / 4) * (OW / 32), jp_cdiv(Cin, 128), 1),
                                   dim3(256), 0, st, wq, dy, e, Cin, Cout, NST, OH, OW, xam);
            jp_prof_after(st);
            JP_LAUNCH_CHECK();
        }
        if (KH == 1 && stride == 2 && pad == 0 && H % 2 == 0 && W % 2 == 0 && 2 * OH == H && 2 * OW == W && p1s2_ok(Cin, Cout, N, OH, OW)) {
            // 1x1 stride 2: the stride-1 1x1 kernel over the half-resolution dY, scattering epilogue
            float* wfr = ws + dgrad_tap_floats(Cin, Cout, KH);
            const int bmt = p9_bmt(Cin, 1, p9_ptiles(N, OH, OW));
            if (!ws_state) pack_p9(w, wfr, Cout, Cin, 1, bmt, 1, st);
            DgradS2PointEpi ep{dx, Cin, OH * OW, OW, accumulate};
            launch_p9s<false, false, DgradS2PointEpi, 1>(wfr, dy, ep, Cin, Cout, N, OH, OW, st, 0, bmt);
            JP_LAUNCH_CHECK();
        }
        if (!ws_state && !p9_only) pack_weights(w, ws, Cout, Cin, KH * KH, Cp, 1, st);
        PackA a{ws, Cin, Kp, Cp, KH * KH};
        if (KH == 3 && stride == 2 && pad == 1 && pad_mode != JP_PAD_REFLECT && H % 2 == 0 && W % 2 == 0 && Nc % 256 == 0 &&
            2 * OH == H && 2 * OW == W) {
            // parity-class form: 4 tap slots instead of 9 taps per input pixel
            PackAS2 a2{ws, Cin, Cp, (int)Nc};
            DgradS2B b2{dy, Cp, (int)Nc, H / 2, W / 2, Cout, OH, OW};
            DgradS2Epi e2{dx, Cin, (int)Nc, H / 2, W / 2, accumulate};
            launch_auto(a2, b2, e2, Cin, (int)npix, 4 * Cp, 1, 4 * Cp, st);
            JP_LAUNCH_CHECK();
        }
        JpP9smPlan sm;
        if (!dgrad_row_tail(Cin) && !(sp <= 1 && p9_only) && p9sm_wanted(Cin, Cout, N, H, W, KH, stride, pad, &sm) && (sm.splits == 1 || split_ws)) {
            // small maps: main pass on the split-bf16 patch kernel (taps mirrored, zero fill), then the reflection fold as usual
            float* wfr = ws + dgrad_tap_floats(Cin, Cout, KH);
            if (!ws_state) pack_p9(w, wfr, Cout, Cin, 1, sm.bmt, KH * KH, st);
            jp_p9sm_launch(sm, wfr, dy, dx, nullptr, JP_ACT_NONE, accumulate, split_ws, Cin, Cout, N, H, W, KH * KH, 0, 1, st);
            if (sm.splits > 1) slice_reduce_nchw(split_ws, dx, nullptr, Cin, (int)npix, H * W, sm.splits, JP_ACT_NONE, accumulate, st);
        } else
        if (sp > 1 && split_ws) {   // small grids: K slices to scratch, fixed-order reduction (no memset, no atomics)
            const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
            WgradEpiWS es{split_ws, Cin, (int)npix};
            JP_KH_SWITCH(KH, {
                DgradBT<KH_> b{dy, Cp, (int)npix, H, W, Cout, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
                launch_auto(a, b, es, Cin, (int)npix, Kp, jp_cdiv(Kp, kps), kps, st);
            });
            slice_reduce_nchw(split_ws, dx, nullptr, Cin, (int)npix, H * W, jp_cdiv(Kp, kps), JP_ACT_NONE, accumulate, st);
        } else if (sp > 1) {
            const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
            if (!accumulate) JP_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)npix * Cin, st));
            AtomicEpi ea{dx, Cin, H * W};
            JP_KH_SWITCH(KH, {
                DgradBT<KH_> b{dy, Cp, (int)npix, H, W, Cout, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
                launch_auto(a, b, ea, Cin, (int)npix, Kp, jp_cdiv(Kp, kps), kps, st);
            });
        } else {
            // the main launch covers the first Mm rows; a row tail is finished by its own launch on the same pack
            const int tail = dgrad_row_tail(Cin), Mm = Cin - tail;
            auto launch_tail = [&](auto b) {
                if (!tail) return;
                PackA at{ws + (size_t)Mm * Cp, Cin, Kp, Cp, KH * KH};
                DgradEpi et{dx + (size_t)Mm * H * W, Cin, H * W, accumulate};
                launch_auto(at, b, et, tail, (int)npix, Kp, 1, Kp, st);
            };
            if (stride == 1) {
                JP_KH_SWITCH(KH, {
                    DgradBT<KH_, true> b{dy, Cp, (int)npix, H, W, Cout, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
                    const int bn3 = Mm <= 64 ? 256 : 128;
                    if (KH == 1 && pad == 0 && tail == 0 && p9_ok(Cin, Cout, N, H, W, 1)) {
                        float* wfr = ws + dgrad_tap_floats(Cin, Cout, KH);
                        if (!ws_state) pack_p9(w, wfr, Cout, Cin, 1, p9_bmt(Cin, 1, p9_ptiles(N, H, W)), 1, st);
                        launch_p1(wfr, dy, e, Cin, Cout, N, H, W, st);
                    } else
                    if (KH == 3 && pad == 1 && (tail == 0 || Mm > 64) && p9_ok(Mm, Cout, N, H, W)) {
                        // P9 patch kernel on dY (taps mirrored, zero fill; the reflection fold stays with the border pass);
                        // fragment-order pack behind the tap-major one (which the border pass still reads).  With a short
                        // row tail (513 = 4*128 + 1) the kernel runs the full 128-row tiles of the same pack, the tail
                        // its own launch below.
                        float* wfr = ws + dgrad_tap_floats(Cin, Cout, KH);
                        if (!ws_state) pack_p9(w, wfr, Cout, Cin, 1, p9_bmt(Cin, 9, p9_ptiles(N, H, W)), 9, st);
                        launch_p9<false, true>(wfr, dy, e, Mm, Cout, N, H, W, st, 0, Cin);
                    } else
                    if (KH == 3 && pad == 1 && Cout >= 32 && W % bn3 == 0 && npix > 64) {
                        // row-tile kernel on dY (taps mirrored, zero fill; the reflection fold stays with the border pass)
                        const Src3 sdy = make_src(dy, Cout, 0, nullptr, 0, 0, nullptr, 0, 0, H, W);
                        if (Mm <= 64) { FwdBR3<false, true, 256> b3{sdy, H, W}; launch_r3<1, 4>(a, b3, e, Mm, (int)npix, Kp, st); }
                        else { FwdBR3<false, true, 128> b3{sdy, H, W}; launch_r3<2, 2>(a, b3, e, Mm, (int)npix, Kp, st); }
                    } else
                    launch_auto(a, b, e, Mm, (int)npix, Kp, 1, Kp, st);
                    launch_tail(b);
                });
            } else
            JP_KH_SWITCH(KH, {
                DgradBT<KH_> b{dy, Cp, (int)npix, H, W, Cout, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
                launch_auto(a, b, e, Mm, (int)npix, Kp, 1, Kp, st);
                launch_tail(b);
            });
        }
        if (pad_mode == JP_PAD_REFLECT)     // fold the reflected ring back in (border-adjacent lines only)
            border_pass(a, dy, dx, Cin, Cp, Kp, Cout, N, H, W, split_ws, st);
    } else {
        const int K = Cout * KH * KH;
        JP_KH_SWITCH(KH, {
            DgradA<KH_> a{w, Cin, K};
            DgradB<KH_> b{dy, K, (int)npix, H, W, Cout, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
            launch_auto(a, b, e, Cin, (int)npix, K, 1, jp_cdiv(K, KC) * KC, st);
        });
    }
    JP_LAUNCH_CHECK();
}


// per-source dgrad of a conv whose input is the channel concat of up to 3 sources, one of them read through the fused
// nearest-2x upsample: gradients go straight into the sources' own buffers (dx_s: (N, c_s, H, W), or (N, c_s, H/2, W/2)
// for the upsampled one; NULL = not needed; acc_s: add instead of overwrite) -- no concat-sized gradient tensor.
static bool dgrad_segments_ok(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W, int Cout, int KH,
                              int stride, int pad, int pad_mode) {
    const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2};
    int nup = 0;
    for (int i = 0; i < 3; ++i)
        if (cs[i] && us[i]) { ++nup; if (cs[i] < 32) return false; }
    return nup == 1 && KH == 3 && stride == 1 && pad == 1 && pad_mode == JP_PAD_REFLECT && H % 2 == 0 && W % 2 == 0 && H >= 4 &&
           W >= 4 && Cout >= 16 && (long)N * H * W < (1L << 31) && (long)N * (H / 2) * (W / 2) / 128 >= 96;
}
extern "C" int jp_conv2d_dgrad_src3_ok(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W, int Cout,
                                       int KH, int stride, int pad, int pad_mode) {
    if (up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W)) return 1;
    return dgrad_segments_ok(c0, up0, c1, up1, c2, up2, N, H, W, Cout, KH, stride, pad, pad_mode) ? 1 : 0;
}
// scratch for jp_conv2d_dgrad_src3's `split_ws`: <= 4 K slices of the widest full-resolution segment's border pass
extern "C" long jp_conv2d_dgrad_src3_split_floats(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W) {
    const int cm = std::max(std::max(up0 ? 0 : c0, up1 ? 0 : c1), up2 ? 0 : c2);
    const int cu = std::max(std::max(up0 ? c0 : 0, up1 ? c1 : 0), up2 ? c2 : 0);
    // <= 4 slices of a full-resolution segment's border pass, <= 8 slices of the upsampled segment's edge pass (N * (H + W) pixels)
    return std::max(4L * cm * N * (2L * H + 2L * W), 8L * cu * N * ((long)H + W));
}

extern "C" int jp_conv2d_dgrad_src3(const float* dy, const float* w, float* dx0, int c0, int up0, int acc0, float* dx1,
                                    int c1, int up1, int acc1, float* dx2, int c2, int up2, int acc2, int N, int H, int W,
                                    int Cout, int KH, int stride, int pad, int pad_mode, float* ws, int ws_state,
                                    float* split_ws, const float* amax_dy, float* amax_dx0, int* amax_dx0_done, float* amax_ws,
                                    void* stream) {
    if (amax_dx0_done) *amax_dx0_done = 0;
    // split_ws: optional scratch of jp_conv2d_dgrad_src3_split_floats floats for the border passes (NULL: read-modify-write epilogue)
    JP_CHECK_ARG(dy && w, "conv2d_dgrad_src3: null pointer");
    if (up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W)) {
        if (dx0) jp_up_head_dgrad(dy, w, dx0, N, c0, H / 2, W / 2, acc0, (hipStream_t)stream);
        JP_LAUNCH_CHECK();
    }
    JP_CHECK_ARG(ws != nullptr, "conv2d_dgrad_src3: null scratch");
    JP_CHECK_ARG(dgrad_segments_ok(c0, up0, c1, up1, c2, up2, N, H, W, Cout, KH, stride, pad, pad_mode),
                 "conv2d_dgrad_src3: shape not supported (check jp_conv2d_dgrad_src3_ok)");
    JP_CHECK_ARG(JP_NS != 2 || amax_ws || amax_dy, "conv2d_dgrad_src3"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(dy, amax_dy);
    ax.ws = amax_ws;
    const JpCall st((hipStream_t)stream, &ax);
    const int Cin = c0 + c1 + c2, Cp = pad32(Cout), Kp = 9 * Cp;
    const long npix = (long)N * H * W;
    float* dxs[3] = {dx0, dx1, dx2};
    const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2}, accs[3] = {acc0, acc1, acc2};
    if (!ws_state) pack_weights(w, ws, Cout, Cin, 9, Cp, 1, st);  // [tap][ci][Cp] for the full-resolution segments
    float* wsT = ws + ((size_t)9 * Cin + 256) * Cp;               // [16][Cx][Cp] for the upsampled one
    const int cx_up = up0 ? c0 : (up1 ? c1 : c2);
    DgradBT<3, true> b{dy, Cp, (int)npix, H, W, Cout, H, W, 1, 1, 1};
    int coff = 0;
    bool frag_packed = false;
    for (int sidx = 0; sidx < 3; ++sidx) {
        const int C = cs[sidx];
        if (!C) continue;
        float* dx = dxs[sidx];
        // amax_dx0: max |dx0| out of the first source's passes (main patch kernel + border fold), if it is a full-resolution one
        ax.out = (sidx == 0 && !us[0]) ? reinterpret_cast<unsigned*>(amax_dx0) : nullptr;
        ax.out_taken = false;
        if (dx && !us[sidx]) {
            PackA a{ws + (size_t)coff * Cp, Cin, Kp, Cp, 9};
            if (C <= 4 && (long)C * Cout * 9 * 4 <= 48 * 1024) {
                // a few channels (the disparity channel): direct zero-pad correlation of dY with the flipped taps
                // instead of a 64-row MFMA tile; the reflection fold still comes from the border pass below
                float* wf = wsT + (16L * cx_up + 256) * Cp;     // behind the upsampled segment's pack (+ its slack)
                if (!ws_state) do_pack(PACK_FLIP, w, wf, (long)C * Cout * 9, Cout, Cin, coff, C, 0, 0, st);
                jp_conv_small_fwd(dy, Cout, 0, nullptr, 0, 0, nullptr, 0, 0, wf, nullptr, dx, N, H, W, C, JP_ACT_NONE, 0, st,
                                  accs[sidx]);
            } else {
                DgradEpi e{dx, C, H * W, accs[sidx]};
                const int bn3 = C <= 64 ? 256 : 128;
                if (Cin > 64 && C > 64 && coff % p9_bmt(Cin, 9, p9_ptiles(N, H, W)) == 0 && p9_ok(C, Cout, N, H, W)) {
                    // P9 patch kernel on this segment's 128-row tiles of the whole bank's fragment-order pack
                    float* wfr = ws + dgrad_tap_floats(Cin, Cout, 3);
                    if (!ws_state && !frag_packed) {
                        pack_p9(w, wfr, Cout, Cin, 1, p9_bmt(Cin, 9, p9_ptiles(N, H, W)), 9, st);
                        frag_packed = true;
                    }
                    launch_p9<false, true>(wfr, dy, e, C, Cout, N, H, W, st, coff / p9_bmt(Cin, 9, p9_ptiles(N, H, W)), Cin);
                } else
                if (W % bn3 == 0 && Cout >= 32) {     // row-tile kernel, see jp_conv2d_dgrad
                    const Src3 sdy = make_src(dy, Cout, 0, nullptr, 0, 0, nullptr, 0, 0, H, W);
                    if (C <= 64) { FwdBR3<false, true, 256> b3{sdy, H, W}; launch_r3<1, 4>(a, b3, e, C, (int)npix, Kp, st); }
                    else { FwdBR3<false, true, 128> b3{sdy, H, W}; launch_r3<2, 2>(a, b3, e, C, (int)npix, Kp, st); }
                } else {
                    launch_auto(a, b, e, C, (int)npix, Kp, 1, Kp, st);
                }
            }
            border_pass(a, dy, dx, C, Cp, Kp, Cout, N, H, W, split_ws, st);
            if (sidx == 0 && amax_dx0_done) *amax_dx0_done = ax.out_taken ? 1 : 0;
        } else if (dx) {
            const int h2 = H / 2, w2 = W / 2, KpU = 16 * Cp;
            const long tot = 16L * C * Cp, np2 = (long)N * h2 * w2;
            if (!ws_state) do_pack(PACK_UP_DGRAD, w, wsT, tot, Cout, Cin, coff, C, Cp, 0, st);
            PackA a{wsT, C, KpU, Cp, 16};
            DgradUPB bu{dy, (int)np2, h2, w2, Cout};
            DgradEpi e{dx, C, h2 * w2, accs[sidx]};
            if (p9sd_enabled() && h2 % 4 == 0 && w2 % 32 == 0 && Cout % 16 == 0 && (long)N * Cout * H * W * 4 < (1L << 31) &&
                (long)jp_cdiv(C, 128) * N * (h2 / 4) * (w2 / 32) >= 192) {
                // split-product patch kernel over the full-resolution dY (igemm_p9sd.h); its pack sits behind the P9 one
                float* wsd = ws + dgrad_tap_floats(Cin, Cout, 3) + p9_alloc_floats(Cin, Cp);
                if (!ws_state) do_pack(PACK_SPLITUPD, w, wsd, p9sd_floats(C, Cout), Cout, Cin, coff, C, 0, 0, st);
                const float* xam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * H * W, st) : nullptr;
                jp_prof_before(p9sd_tag<DgradEpi>(), JP_NPROD * 2.0 * C * (double)np2 * 16.0 * Cp, st);
                dim3 grid(N * (h2 / 4) * (w2 / 32), jp_cdiv(C, 128), 1);
                hipLaunchKernelGGL((jp_igemm_p9sd_kernel<DgradEpi>), grid, dim3(256), 0, st, reinterpret_cast<const unsigned*>(wsd), dy, e,
                                   C, Cout, Cp / 16, h2, w2, xam);
                jp_prof_after(st);
            } else
            launch_auto(a, bu, e, C, (int)np2, KpU, 1, KpU, st);
            const int Nb = N * (2 * w2 + 2 * h2);
            DgradUPBorderB bb{dy, Nb, h2, w2, Cout};
            DgradEdgeEpi be{dx, C, h2, w2, Nb, 0};
            const long btiles = (long)jp_cdiv(C, C <= 64 ? 64 : 128) * jp_cdiv(Nb, C <= 64 ? 256 : 128);
            // 16 slots x Cout: a long K loop of branchy gathers on a few dozen tiles -- up to 4 K slices (atomic epilogue)
            const int bsp = (int)std::max<long>(border_splits(btiles, KpU / KC), std::min<long>(4, jp_cdiv(256, btiles)));
            const int bkps = jp_cdiv(jp_cdiv(KpU, bsp), KC) * KC;
            be.split = jp_cdiv(KpU, bkps) > 1;
            if (be.split && split_ws) {
                // K slices to scratch, then one fixed-order fold into dx (round 6: the slices met in float atomics -- run-dependent last
                // bits in the gradient of the upsampled segment, which the whole coarser decoder level inherits)
                const int nsl = std::min(jp_cdiv(KpU, bkps), 8);
                const int wkps = jp_cdiv(jp_cdiv(KpU, nsl), KC) * KC, ns2 = jp_cdiv(KpU, wkps);
                WgradEpiWS es{split_ws, C, Nb};
                launch_auto(a, bb, es, C, Nb, KpU, ns2, wkps, st);
                const long total = (long)C * Nb;
                hipLaunchKernelGGL(edge_add_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, split_ws, dx, C,
                                   Nb, h2, w2, ns2);
            } else
            launch_auto(a, bb, be, C, Nb, KpU, jp_cdiv(KpU, bkps), bkps, st);
        }
        coff += C;
    }
    JP_LAUNCH_CHECK();
}

#ifdef P9S_TRACE   // debug build only (not part of the ABI): cycle stamps of one 1x1 workgroup, tools/debug/p1_trace.py
extern "C" int dbg_p9s_trace(unsigned long long* host40) {
    return (int)hipMemcpyFromSymbol(host40, HIP_SYMBOL(jp_p9s_trace), 64 * sizeof(unsigned long long));   // host buffer: 64 entries
}
#endif
