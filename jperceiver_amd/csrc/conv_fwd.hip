// conv2d forward / dgrad / wgrad for the JPerceiver train step as instances of the fp32-MFMA
// implicit-GEMM engine (igemm.h).  Forward is in this unit, dgrad in conv_dgrad.hip, wgrad in
// conv_wgrad.hip; the patch-kernel launch layer forward and dgrad share is in conv_launch.h, what
// all three use is in conv_common.h.  Replaces every nn.Conv2d /
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
// Loader families (DESIGN.md §4.1 has the measurements behind each), and the unit each lives in:
//   "T"  tap-major fast path: K ordered (channel chunk of 32, tap, channel); tap decode, bounds / reflection and source
//        selection once per chunk; scalar-base addressing (wave-uniform 64-bit base + per-lane 32-bit offset); weights
//        re-packed per launch to [tap][row][channel_pad32] (L2-resident, conv_pack.hip) so the A loads are coalesced.
//        (PackA: conv_launch.h; FwdBT: here; DgradBT and the border / edge passes: conv_dgrad.hip.)
//   "R3" row-tile kernel for 3x3 stride-1 layers whose pixel tile is one image-row segment: the three dx taps share one
//        staged row segment (forward and dgrad main pass).  (FwdBR3, launch_r3: conv_launch.h.)
//   "P"  parity-class kernels for inputs read through the fused nearest-2x upsample (iconv layers, disparity heads):
//        4 pre-summed weight slots per output parity instead of 9 taps, in forward, dgrad and wgrad.
//        (PackAP, FwdBP: here; DgradUPB: conv_dgrad.hip; the wgrad form: conv_wgrad.hip.)
//   "S2" parity-class dgrad of the 3x3 stride-2 convs (conv_dgrad.hip); "C" whole-tap K chunks for the 3/6-channel stems (here).
//   "G"  generic (channel-major K, per-element decode): whatever the fast paths do not cover.
//        (FwdA, FwdB: here; DgradA, DgradB: conv_dgrad.hip; the gather: conv_common.h.)
//
// slice_reduce_nchw_kernel, the fixed-order fold of split-K partials, is launched by both directions through the host function
// slice_reduce_nchw (declared in conv_launch.h, hidden visibility); it is defined here and nowhere else.
#include "conv_launch.h"
#include "igemm_p9us2.h"
#include "igemm_p9s2f.h"
#include "igemm_p7s.h"
#include "igemm_p9u.h"

namespace {

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
template <class E>
const char* p9s2f_tag() { return __PRETTY_FUNCTION__; }
template <int CIN, class E>
const char* p7s_tag() { return __PRETTY_FUNCTION__; }
template <int WM, int WN, class E>
const char* p9sx2_tag() { return __PRETTY_FUNCTION__; }
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
inline bool seg_aligned(int c0, int c1, int c2) {   // every segment end except the last is a multiple of 32
    if (c1 == 0 && c2 == 0) return true;
    if (c0 % 32) return false;
    if (c2 != 0 && (c0 + c1) % 32) return false;
    return true;
}

}  // namespace

// outside the anonymous namespace: conv_dgrad.hip calls it too (declared in conv_launch.h, hidden visibility)
void slice_reduce_nchw(const float* part, float* y, const float* bias, int M, int Npix, int HW, int splits, int act, int accumulate,
                       hipStream_t st) {
    const long total = (long)M * Npix;
    hipLaunchKernelGGL(slice_reduce_nchw_kernel, dim3((int)std::min<long>((total + 255) / 256, 2048)), dim3(256), 0, st, part, y, bias, M,
                       Npix, HW, splits, act, accumulate);
}

extern "C" int jp_conv2d_up_head_ok(int c0, int up0, int c1, int c2, int Cout, int KH, int stride, int pad, int pad_mode, int H,
                                    int W) {
    return up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W) ? 1 : 0;
}

// floats of `bn_stats` scratch for a forward call with OH x OW output maps: 2 sums x Cout x (at most one partial per 2 x 32 output pixels)
extern "C" long jp_conv2d_fwd_bn_stats_floats(int N, int OH, int OW, int Cout) {
    return 2L * Cout * N * jp_cdiv(OH, 2) * jp_cdiv(OW, 32);
}
// floats of caller-owned scratch for the packed-weight fast path (0 = the generic path will be used).
// which: 0 forward, 1 dgrad, 2 wgrad
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

#ifdef P9S_TRACE   // debug build only (not part of the ABI): cycle stamps of one 1x1 workgroup, tools/debug/p1_trace.py
extern "C" int dbg_p9s_trace(unsigned long long* host40) {
    return (int)hipMemcpyFromSymbol(host40, HIP_SYMBOL(jp_p9s_trace), 64 * sizeof(unsigned long long));   // host buffer: 64 entries
}
#endif
