// conv2d wgrad: jp_conv2d_wgrad[_src3], their scratch-size queries, the split-K plans and the reduce / fold kernels, and the loaders
// and epilogues that only wgrad instantiates (conv_fwd.hip's head has the GEMM shapes and the loader families).
// igemm_w9.h, igemm_w9s.h and igemm_w9s2.h define non-template kernels: they are included here and nowhere else.
#include "conv_common.h"
#include "igemm_w9s.h"
#include "igemm_w9s2.h"
#include "igemm_w4s.h"
#include "igemm_w9.h"
#include "igemm_w7.h"
constexpr double JP_NPROD = JP_NS == 2 ? 3.0 : 6.0;     // matrix-pipe products per fp32 product of the W9S-family kernels (as in conv_launch.h)

namespace {

struct WgradASt {
    size_t base;
    int valid;
};
struct WgradA {  // A[m=co][k=pixel] = dY[img][co][pix]
    static constexpr bool ALONG_K = true;
    typedef WgradASt St;
    const float* dy;
    int Cout, Npix, OHW;
    __device__ __forceinline__ void init(St&, int, int) const {}
    __device__ __forceinline__ void fix(St& st, int p) const {
        st.valid = p < Npix;
        int img = p / OHW;
        st.base = (size_t)img * Cout * OHW + (p - img * OHW);
    }
    __device__ __forceinline__ float get(const St& st, int m, int) const {
        return (st.valid && m < Cout) ? dy[st.base + (size_t)m * OHW] : 0.f;
    }
};

template <int KH>
struct WgradB {  // B[k=pixel][n=(ci,dy,dx)] = xpad[img][ci][oy*s+dy][ox*s+dx]
    static constexpr bool ALONG_K = true;
    typedef PixSt St;
    Src3 src;
    int Kw, Npix, OH, OW, stride, pad, reflect;
    __device__ __forceinline__ void init(St&, int, int) const {}
    __device__ __forceinline__ void fix(St& st, int p) const { st = conv_pix(p, Npix, OH, OW, stride, pad); }
    __device__ __forceinline__ float get(const St& st, int j, int) const {
        if (!st.valid || j >= Kw) return 0.f;
        return conv_gather<KH>(src, st, j, reflect);
    }
};

struct WgradEpi {  // dw[co][j] += acc   (split-K partials meet in L2 atomics)
    typedef int St;
    float* dw;
    int Kw;
    __device__ __forceinline__ St col(int n) const { return n; }
    __device__ __forceinline__ void put(St j, int m, float v) const { atomicAdd(dw + (size_t)m * Kw + j, v); }
};

// ---- wgrad of the upsampled segment in the same parity-class form: dW'_{class}[slot][co][c] = sum over the class's
// output pixels of dY[co][2i+a][2j+b] * X[c][clamp(i-1+a+r)][clamp(j-1+b+s)]  (GEMM M=co, N=(class, slot, c), K = class
// pixels; 4/9 of the plain wgrad's MFMA work), then dW[dy][dx] += the 4 (class, slot) pairs that contain the tap.
// Preconditions: W/2 % 32 == 0 (a K chunk is 32 consecutive j of one row), Cx % 128 == 0, Cout % 8 == 0.
struct WgradAPSt {
    const float* base;
    unsigned voff;
    int a, b;
};
struct WgradAP {  // A[m=co][k=(img,i,j) of the tile's class] = dY[img][co][2i+a][2j+b]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool WANTS_TILE = true;
    typedef WgradAPSt St;
    const float* dy;
    int Cout, h2, w2, ncls;    // ncls = columns per class = 4 * Cx
    __device__ __forceinline__ void init(St& st, int, int, int, int n0) const {
        const int cls = n0 / ncls;
        st.a = cls >> 1;
        st.b = cls & 1;
        st.base = dy;
        st.voff = ((threadIdx.x >> 5) * (4 * h2 * w2) + 2 * (threadIdx.x & 31)) * 4u;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const int p0 = __builtin_amdgcn_readfirstlane(p & ~31);
        const int hw2 = h2 * w2;
        const int img = p0 / hw2, rem = p0 - img * hw2;
        const int i = rem / w2, j0 = rem - i * w2;
        st.base = dy + (size_t)img * Cout * (4 * hw2) + (size_t)(2 * i + st.a) * (2 * w2) + 2 * j0 + st.b;
    }
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)min(m_u, Cout - 8) * (4 * h2 * w2);
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};
struct WgradBPSt {
    const float* base;
    unsigned voff;
    int a, b, r, s, c0;
};
struct WgradBP {  // B[k=(img,i,j)][n=(class, slot, c)] = X[img][c][clamp(i-1+a+r)][clamp(j-1+b+s)]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool WANTS_TILE = true;
    typedef WgradBPSt St;
    const float* x;     // half-resolution source (N, Cx, h2, w2)
    int Cx, h2, w2;
    __device__ __forceinline__ void init(St& st, int, int, int, int n0) const {
        const int q = n0 / Cx;           // (class, slot)
        st.c0 = n0 - q * Cx;
        const int cls = q >> 2, slot = q & 3;
        st.a = cls >> 1; st.b = cls & 1; st.r = slot >> 1; st.s = slot & 1;
        st.base = x;
        st.voff = 0;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const int p0 = __builtin_amdgcn_readfirstlane(p & ~31);
        const int hw2 = h2 * w2;
        const int img = p0 / hw2, rem = p0 - img * hw2;
        const int i = rem / w2;
        const int j = p - img * hw2 - i * w2;       // per lane
        const int xi = min(max(i - 1 + st.a + st.r, 0), h2 - 1);
        const int xj = min(max(j - 1 + st.b + st.s, 0), w2 - 1);
        st.voff = (unsigned)((threadIdx.x >> 5) * hw2 + xj) * 4u;
        st.base = x + (size_t)(img * Cx + st.c0) * hw2 + (size_t)xi * w2;
    }
    __device__ __forceinline__ float get_u(const St& st, int, int r) const {
        const float* rp = st.base + (size_t)(8 * r) * (h2 * w2);
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};
// dw[m][c_off + c][tap] += sum over splits and over the 4 (class, slot) pairs containing the tap of ws[k][m][n]
__global__ void wgrad_fold_parity_kernel(const float* __restrict__ ws, float* __restrict__ dw, int M, int Cx, int splits,
                                         int c_off, int Ctot) {
    const long total = (long)M * Cx * 9, plane = (long)M * 16 * Cx;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cx);
        const long t = i / Cx;
        const int tap = (int)(t % 9), m = (int)(t / 9);
        const int dy = tap / 3, dx = tap - dy * 3;
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int r = a ? (dy == 2) : (dy >= 1);
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int sx = b ? (dx == 2) : (dx >= 1);
                const long n = (long)(((a * 2 + b) * 4 + r * 2 + sx)) * Cx + c;
                for (int k = 0; k < splits; ++k) s += ws[(size_t)k * plane + (size_t)m * 16 * Cx + n];
            }
        }
        dw[((size_t)m * Ctot + c_off + c) * 9 + tap] += s;
    }
}

template <int KH>
struct WgradBT {  // B[k=pixel][n=(tap,ci)], any source layout (per-element decode)
    static constexpr bool ALONG_K = true;
    typedef PixSt St;
    Src3 src;
    int Np, Cp, Cin, Npix, OH, OW, stride, pad, reflect;
    unsigned magic;   // floor(2^32 / Cp) + 1: n / Cp == umulhi(n, magic) for n < 2^16
    __device__ __forceinline__ void init(St&, int, int) const {}
    __device__ __forceinline__ void fix(St& st, int p) const { st = conv_pix(p, Npix, OH, OW, stride, pad); }
    __device__ __forceinline__ float get(const St& st, int n, int) const {
        if (!st.valid || n >= Np) return 0.f;
        const int tap = (Cp == 1 ? n : (int)__umulhi((unsigned)n, magic));
        const int ci = n - tap * Cp;
        if (ci >= Cin) return 0.f;
        const int dy = tap / KH, dx = tap - dy * KH;
        int iy = st.iy0 + dy, ix = st.ix0 + dx;
        if (reflect) {
            iy = jp_reflect(iy, src.H);
            ix = jp_reflect(ix, src.W);
        } else if ((unsigned)iy >= (unsigned)src.H || (unsigned)ix >= (unsigned)src.W) {
            return 0.f;
        }
        return src.at(st.img, ci, iy, ix);
    }
};

// single full-resolution source: the (tap, ci) decode of every slot is done ONCE per thread (the N index of a
// slot never changes over the K loop), leaving ~8 integer ops per gathered element.
struct WgradB1St {
    PixSt px;
    const float* base;   // x + img*Cin*H*W
    int off[32];         // ci*H*W, or -1 for padded / out-of-range slots
    int dd[32];          // dy | dx << 8
};

template <int KH>
struct WgradBT1 {
    static constexpr bool ALONG_K = true;
    typedef WgradB1St St;
    const float* x;      // already offset to the first channel of the sub-range
    int Np, Cp, Cin, Ctot, H, W, Npix, OH, OW, stride, pad, reflect;   // Cin = channels in this sub-range
    unsigned magic;
    __device__ __forceinline__ void init(St& st, int n_first, int step) const {
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int n = n_first + step * r;
            const int tap = (Cp == 1 ? n : (int)__umulhi((unsigned)n, magic));
            const int ci = n - tap * Cp;
            const int dy = tap / KH, dx = tap - dy * KH;
            st.off[r] = (n < Np && ci < Cin) ? ci * H * W : -1;
            st.dd[r] = dy | (dx << 8);
        }
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        st.px = conv_pix(p, Npix, OH, OW, stride, pad);
        st.base = x + (size_t)st.px.img * Ctot * H * W;
    }
    __device__ __forceinline__ float get(const St& st, int, int r) const {
        if (!st.px.valid || st.off[r] < 0) return 0.f;
        int iy = st.px.iy0 + (st.dd[r] & 255), ix = st.px.ix0 + (st.dd[r] >> 8);
        if (reflect) {
            iy = jp_reflect(iy, H);
            ix = jp_reflect(ix, W);
        } else if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) {
            return 0.f;
        }
        return st.base[st.off[r] + iy * W + ix];
    }
};

// Channel counts that are multiples of the N tile (128): every workgroup's N tile lies inside ONE filter tap, so
// the tap shift, bounds / reflection and the source pointer are per-chunk work and each element is one strided load
// (same cost as the forward gather, ~100 fewer VGPRs than the table version -> 3 waves/SIMD).
struct WgradBUSt {
    const float* q;   // x element (first slot's channel) at this chunk's pixel shifted by the tile's tap
    int dy, dx, c0, ok, step;
};
template <int KH>
struct WgradBU {
    static constexpr bool ALONG_K = true;
    typedef WgradBUSt St;
    const float* x;
    int Cpp, Cin, Ctot, H, W, Npix, OH, OW, stride, pad, reflect;
    __device__ __forceinline__ void init(St& st, int n_first, int step) const {
        st.step = step;
        const int tap = n_first / Cpp;          // Cpp % tile == 0: identical for every slot of the workgroup
        st.c0 = n_first - tap * Cpp;
        st.dy = tap / KH;
        st.dx = tap - st.dy * KH;
        st.q = nullptr;
        st.ok = 0;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const PixSt px = conv_pix(p, Npix, OH, OW, stride, pad);
        int iy = px.iy0 + st.dy, ix = px.ix0 + st.dx;
        st.ok = px.valid;
        if (reflect) {
            iy = jp_reflect(iy, H);
            ix = jp_reflect(ix, W);
        } else if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) {
            st.ok = 0;
        }
        if (st.ok) st.q = x + ((size_t)(px.img * Ctot + st.c0) * H + iy) * W + ix;
    }
    __device__ __forceinline__ float get(const St& st, int, int r) const {
        // slot r holds channel c0 + step*r (step = slot stride of the lanes-along-K mapping)
        return (st.ok && st.c0 + st.step * r < Cin) ? st.q[(size_t)(st.step * r) * H * W] : 0.f;
    }
};

// ---- scalar-base wgrad loaders (igemm.h SPLIT protocol).  Preconditions (host-checked): OH*OW % 32 == 0, so a
// K chunk of 32 pixels never straddles two images (the image and the chunk's first pixel are wave-uniform), and
// Cout % 8 == 0, so the 8-row slot groups can be clamped with scalar arithmetic.
struct WgradASSt {
    const float* base;   // uniform: dY (image of the chunk, channel 0, first pixel of the chunk)
    unsigned voff;       // per-lane: (row within the slot group, pixel within the chunk), constant
};
struct WgradAS {  // A[m=co][k=pixel] = dY[img][co][pix]
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    typedef WgradASSt St;
    const float* dy;
    int Cout, Npix, OHW, P;   // P = pixels per image padded to 32: K = (img, padded pixel), the padding is masked on B
    __device__ __forceinline__ void init(St& st, int, int) const {
        st.base = dy;
        st.voff = ((threadIdx.x >> 5) * OHW + (threadIdx.x & 31)) * 4u;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const int p0 = __builtin_amdgcn_readfirstlane(p & ~31);
        const int img = p0 / P, pix0 = p0 - img * P;
        st.base = dy + (size_t)img * Cout * OHW + pix0;
        // lanes in the per-image K padding re-read the last pixel (their B operand is zeroed)
        st.voff = ((threadIdx.x >> 5) * OHW + min((int)(threadIdx.x & 31), OHW - 1 - pix0)) * 4u;
    }
    __device__ __forceinline__ float get_u(const St& st, int m_u, int) const {
        const float* rp = st.base + (size_t)min(m_u, Cout - 8) * OHW;   // rows >= Cout: duplicates, never stored
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
};

// uniform-tap B gather (Cin % 128 == 0, 128-wide N tile -> one filter tap per workgroup), scalar-base form
struct WgradBUSSt {
    int dy, dx, c0;      // uniform: the tile's tap and first channel
    const float* base;   // uniform: x (image of the chunk, channel c0)
    unsigned voff;       // per-lane: (channel within the slot group, tap-shifted pixel)
    int ok;
};
template <int KH, bool REFLECT>
struct WgradBUS {
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool POST = true;
    typedef WgradBUSSt St;
    const float* x;
    int Cpp, Ctot, H, W, OH, OW, stride, pad, P;
    __device__ __forceinline__ void init(St& st, int n_first, int) const {
        const int n0 = __builtin_amdgcn_readfirstlane(n_first - (int)(threadIdx.x >> 5));
        const int tap = n0 / Cpp;
        st.c0 = n0 - tap * Cpp;
        st.dy = tap / KH;
        st.dx = tap - st.dy * KH;
        st.base = x;
        st.voff = 0;
        st.ok = 1;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const int ohw = OH * OW;
        const int p0 = __builtin_amdgcn_readfirstlane(p & ~31);
        const int img = p0 / P;                         // uniform
        const int pr = p - img * P;
        const int pix = min(pr, ohw - 1);
        const int oy = pix / OW, ox = pix - oy * OW;
        int iy = oy * stride - pad + st.dy, ix = ox * stride - pad + st.dx;
        st.ok = pr < ohw;                               // per-image K padding
        if (REFLECT) {
            iy = jp_reflect(iy, H);
            ix = jp_reflect(ix, W);
        } else {
            st.ok = st.ok && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            iy = min(max(iy, 0), H - 1);
            ix = min(max(ix, 0), W - 1);
        }
        st.voff = (unsigned)(((threadIdx.x >> 5) * H + iy) * W + ix) * 4u;
        st.base = x + (size_t)(img * Ctot + st.c0) * H * W;
    }
    __device__ __forceinline__ float get_u(const St& st, int, int r) const {   // slot r = channel c0 + 8r (+ lane part)
        const float* rp = st.base + (size_t)(8 * r) * H * W;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok); }
    __device__ __forceinline__ float post(const St& st, float v, int) const { return st.ok ? v : 0.f; }
};

// CPT-channel inputs (CPT = 16, 32 or 64): a CPT*TPT wide N tile holds TPT whole filter taps, and slot group r (8
// columns) belongs to tap slot 8r/CPT at compile time -> one per-lane offset per tap per chunk, every element one
// scalar-base load.
template <int TPT>
struct WgradBMSSt {
    int tap0;            // uniform: first tap of the tile
    const float* base;   // uniform: x (image of the chunk, first channel of the sub-range)
    unsigned voff[TPT];  // per-lane: (channel within the slot group, pixel shifted by tap slot s)
    unsigned ok;         // per-lane bit s: tap slot s lies inside the image (zero padding)
};
template <int KH, bool REFLECT, int TPT, int CPT>
struct WgradBMS {
    static constexpr bool ALONG_K = true;
    static constexpr bool SPLIT = true;
    static constexpr bool POST = true;
    typedef WgradBMSSt<TPT> St;
    const float* x;      // already offset to the first channel of the CPT-channel sub-range
    int Ctot, H, W, OH, OW, stride, pad, P;
    __device__ __forceinline__ void init(St& st, int n_first, int) const {
        const int n0 = __builtin_amdgcn_readfirstlane(n_first - (int)(threadIdx.x >> 5));
        st.tap0 = n0 / CPT;
        st.base = x;
        st.ok = ~0u;
#pragma unroll
        for (int s = 0; s < TPT; ++s) st.voff[s] = 0;
    }
    __device__ __forceinline__ void fix(St& st, int p) const {
        const int ohw = OH * OW;
        const int p0 = __builtin_amdgcn_readfirstlane(p & ~31);
        const int img = p0 / P;                         // uniform
        const int pr = p - img * P;
        const int pix = min(pr, ohw - 1);
        const int oy = pix / OW, ox = pix - oy * OW;
        const int by = oy * stride - pad, bx = ox * stride - pad;
        unsigned ok = 0;
#pragma unroll
        for (int s = 0; s < TPT; ++s) {
            const int tap = min(st.tap0 + s, KH * KH - 1);   // taps past the filter: duplicate columns, never stored
            const int dy = tap / KH, dx = tap - dy * KH;
            int iy = by + dy, ix = bx + dx;
            if (REFLECT) {
                ok |= 1u << s;
                iy = jp_reflect(iy, H);
                ix = jp_reflect(ix, W);
            } else {
                ok |= (unsigned)((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) << s;
                iy = min(max(iy, 0), H - 1);
                ix = min(max(ix, 0), W - 1);
            }
            st.voff[s] = (unsigned)(((threadIdx.x >> 5) * H + iy) * W + ix) * 4u;
        }
        st.ok = pr < ohw ? ok : 0u;                     // per-image K padding
        st.base = x + (size_t)img * Ctot * H * W;
    }
    __device__ __forceinline__ float get_u(const St& st, int, int r) const {
        const float* rp = st.base + (size_t)((8 * r) % CPT) * H * W;
        return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rp) + st.voff[(8 * r) / CPT]);
    }
    static constexpr bool ALL_OK = true;
    __device__ __forceinline__ bool all_ok(const St& st) const { return __all(st.ok == ((1u << TPT) - 1u)); }
    __device__ __forceinline__ float post(const St& st, float v, int r) const {
        return ((st.ok >> ((8 * r) / CPT)) & 1u) ? v : 0.f;
    }
};

struct WgradEpiT {  // dw[co][c_off + ci][tap] += acc for n = tap*Cp + ci
    typedef int St;
    float* dw;
    int Cp, Cin, KHW, c_off, Ctot;
    unsigned magic;
    __device__ __forceinline__ St col(int n) const {
        const int tap = (Cp == 1 ? n : (int)__umulhi((unsigned)n, magic));
        const int ci = n - tap * Cp;
        return ci < Cin ? (c_off + ci) * KHW + tap : -1;
    }
    __device__ __forceinline__ void put(St j, int m, float v) const {
        if (j >= 0) atomicAdd(dw + (size_t)m * Ctot * KHW + j, v);
    }
};

// dw[m][c_off + ci][tap] += sum_s ws[s][m][n = tap*Cp + ci]
__global__ void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int M, int Np, int splits,
                                    int Cp, int Cin, int KHW, int c_off, int Ctot) {
    const long total = (long)M * Np;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int m = (int)(i / Np), n = (int)(i - (long)m * Np);
        const int tap = n / Cp, ci = n - tap * Cp;
        if (ci >= Cin) continue;
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += ws[(size_t)k * total + i];
        dw[((size_t)m * Ctot + c_off + ci) * KHW + tap] += s;
    }
}

// W9 partials (Np % 4 == 0, Cp == Cin): 4 consecutive n per thread as one 16-byte load per slice, SL slice lanes per output
// quad (blockDim = 64 x SL) so that few-output / many-slice layers still put enough loads in flight
template <int SL>
__global__ __launch_bounds__(64 * SL) void wgrad_reduce4_kernel(const float* __restrict__ ws, float* __restrict__ dw, int M,
                                                               int Np, int splits, int Cp, int KHW, int c_off, int Ctot) {
    __shared__ float4 part[SL][64];
    const long total4 = (long)M * Np / 4;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long i4 = (long)blockIdx.x * 64 + tx;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < total4) {
        const float4* p = reinterpret_cast<const float4*>(ws) + i4;
#pragma unroll 4
        for (int k = ty; k < splits; k += SL) {
            const float4 v = p[(long)k * total4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    if (SL > 1) {
        part[ty][tx] = s;
        __syncthreads();
        if (ty != 0) return;
#pragma unroll
        for (int k = 1; k < SL; ++k) { const float4 v = part[k][tx]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    }
    if (i4 < total4) {
        const long i = i4 * 4;
        const int m = (int)(i / Np), n = (int)(i - (long)m * Np);
        const int tap = n / Cp, ci = n - tap * Cp;          // the 4 values share the tap (Cp % 4 == 0)
        float* q = dw + ((size_t)m * Ctot + c_off + ci) * KHW + tap;
        q[0] += s.x; q[KHW] += s.y; q[2 * KHW] += s.z; q[3 * KHW] += s.w;
    }
}

// many slices, few outputs (narrow layers: 16x144 outputs x ~700 slices): 64 outputs x 16 slice lanes per workgroup
__global__ __launch_bounds__(1024) void wgrad_reduce_wide_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                 int M, int Np, int splits, int Cp, int Cin, int KHW,
                                                                 int c_off, int Ctot) {
    __shared__ float part[16][65];
    const long total = (long)M * Np;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + tx;
    float s = 0.f;
    if (i < total)
        for (int k = ty; k < splits; k += 16) s += ws[(size_t)k * total + i];
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && i < total) {
#pragma unroll
        for (int k = 1; k < 16; ++k) s += part[k][tx];
        const int m = (int)(i / Np), n = (int)(i - (long)m * Np);
        const int tap = n / Cp, ci = n - tap * Cp;
        if (ci < Cin) dw[((size_t)m * Ctot + c_off + ci) * KHW + tap] += s;
    }
}

// split-K plan of a wgrad GEMM (M x Np, K = npix): workgroups run in rounds of `slots` = 256 CUs x per_cu; a split
// costs its K chunks plus an epilogue -- ~14 chunk-times when the partial tile is merged with device-scope atomics,
// ~3 when it is stored to scratch and summed by wgrad_reduce_kernel (whose pass over splits*M*Np floats is charged
// too).  Returns the split count minimising rounds * (chunks per split + epilogue).
struct WgradPlan {
    int splits, kps;
    bool use_ws;
    long ws_need;
};
inline WgradPlan wgrad_plan(int M, int Np, long npix, int BM, int BN, int per_cu, long ws_floats) {
    const long tiles = (long)jp_cdiv(M, BM) * jp_cdiv(Np, BN), chunks = jp_cdiv(npix, KC), slots = 256L * per_cu;
    WgradPlan best{1, (int)(chunks * KC), false, 0};
    double bc = 1e30;
    for (long sp = 1; sp <= std::max<long>(1, chunks / 4) && sp <= 4096; ++sp) {
        const long per = jp_cdiv(chunks, sp), need = sp * (long)M * Np;
        const double rounds = (double)jp_cdiv(sp * tiles, slots);
        const double c_at = rounds * (per + 14.0);
        if (c_at < bc * 0.999) { bc = c_at; best = WgradPlan{(int)sp, (int)(per * KC), false, 0}; }
        if (sp > 1 && need <= ws_floats) {
            const double c_ws = rounds * (per + 3.0) + (need * 4.0 / 3.0e12 + 6e-6) / 7e-6;
            if (c_ws < bc * 0.999) { bc = c_ws; best = WgradPlan{(int)sp, (int)(per * KC), true, need}; }
        }
    }
    best.splits = jp_cdiv(npix, best.kps);
    return best;
}

// ---- W9 patch wgrad (igemm_w9.h): 3x3 s1 p1, single full-resolution source, >= 128 output channels, input channels a
// multiple of 64.  One 12-wave workgroup per CU: the K (pixel-tile) range is split so that ~256 workgroups exist.
static bool w9_enabled() {
    static const bool on = [] { const char* e = getenv("JP_W9"); return !(e && e[0] == '0'); }();
    return on;
}
// W9S (igemm_w9s.h): the wide variant (> 64 output channels) with split-bf16 products on the bf16 matrix pipe; JP_W9S=0
// keeps the exact-fp32 W9 kernel.  Its pixel tiles are W9S_TR rows high.
constexpr int W9S_TR = 2;
constexpr int W9S_TRN = 4;     // narrow variant (<= 64 output channels): two K groups of 2 rows each
// pixel-tile height of the 256x32-channel variant (NCB = 1): JP_W9S_TR1 = 2 | 4
static inline int w9s_tr1() {
    static const int v = [] { const char* e = getenv("JP_W9S_TR1"); return e ? atoi(e) : 4; }();
    return v == 2 ? 2 : 4;      // 4 (default): 1.5x instead of 2x patch re-staging, half the barriers: 2.738 -> 2.649 ms @256^2 (r04_w9s_ab.log)
}
static bool w9s_enabled() {
    static const bool on = [] { const char* e = getenv("JP_W9S"); return !(e && e[0] == '0'); }();
    return on;
}
struct W9Plan { int splits, tps, ntiles, slices, narrow, split_mfma, ncb1, tr; long need; };
// W9S with 256 output x 32 input channels per workgroup (igemm_w9s.h NCB = 1) for layers whose output channels fill 256-row tiles;
// JP_W9S_NCB=2 keeps the 128 x 64 tiles of round 3
static inline bool w9s_ncb1(int Cout, int narrow) {
    static const bool on = [] { const char* e = getenv("JP_W9S_NCB"); return !(e && e[0] == '2'); }();
    return on && !narrow && Cout % 256 == 0;
}
static inline bool w9_plan(int N, int Cm, int H, int W, int Cout, int KH, int stride, int pad, long ws_floats, W9Plan* p) {
    if (!w9_enabled() || KH != 3 || stride != 1 || pad != 1 || W % 32 || Cm < 64 || Cm % 64 || Cout < 48 ||
        (long)N * Cout * H * W * 4 >= (1L << 31))
        return false;
    const int narrow = Cout <= 64;                    // KG = 2: two K groups per workgroup, two slices per split
    p->split_mfma = w9s_enabled();
    p->ncb1 = p->split_mfma && w9s_ncb1(Cout, narrow);
    // pixel-tile height of the kernel that will run; the 256 x 32 variant falls back from 4-row to 2-row tiles on maps whose height is
    // not a multiple of 4 (round 6: the 10 x 32 and 20 x 64 maps of the 1024 x 320 shape used to drop to the exact-fp32 engine here)
    p->tr = !p->split_mfma ? W9_TR : (narrow ? W9S_TRN : (p->ncb1 ? ((w9s_tr1() == 4 && H % 4 == 0) ? 4 : 2) : W9S_TR));
    if (H % p->tr) return false;
    const int ntiles = N * (H / p->tr) * (W / 32), kg = narrow ? 2 : 1;
    const long out_tiles = p->ncb1 ? (long)(Cm / 32) * (Cout / 256) : (long)(Cm / 64) * jp_cdiv(Cout, narrow ? 64 : 128);
    const long per = (long)Cout * 9 * Cm;
    static const long wgs = [] { const char* e = getenv("JP_W9_WGS"); return e ? atol(e) : 256L; }();
    long sp = std::max<long>(1, std::min<long>(wgs / std::max<long>(1, out_tiles), ntiles / 2));
    sp = std::min<long>(sp, ws_floats / (per * kg));
    if (sp < 1 || ntiles < 8) return false;
    const int tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, tps);
    p->tps = tps;
    p->ntiles = ntiles;
    p->narrow = narrow;
    p->slices = p->splits * kg;
    p->need = (long)p->slices * per;
    return true;
}
// W9S2 (igemm_w9s2.h): the 3x3 stride-2 zero-pad weight gradient of the ResNet stage transitions on the bf16 pipe; JP_W9S2=0 (or
// JP_W9S=0) keeps the exact-fp32 generic engine.
struct W9S2Plan { int splits, tps, ntiles, slices, kg; long need; };
static inline bool w9s2_plan(int N, int Cm, int H, int W, int Cout, int KH, int stride, int pad, int pad_mode, long ws_floats,
                             W9S2Plan* p) {
    static const bool on = [] { const char* e = getenv("JP_W9S2"); return !(e && e[0] == '0'); }();
    if (!on || !w9s_enabled() || KH != 3 || stride != 2 || pad != 1 || pad_mode == JP_PAD_REFLECT || (H & 1) || (W & 1) ||
        (W / 2) % 32 || (H / 2) % 2 || Cm < 32 || Cm % 32 || !(Cout == 128 || Cout % 256 == 0) ||
        (long)N * Cout * (H / 2) * (W / 2) * 4 >= (1L << 31) || (long)N * Cm * H * W * 4 >= (1L << 31))
        return false;
    const int kg = Cout == 128 ? 2 : 1;
    const int ntiles = N * (H / 4) * (W / 64);
    const long out_tiles = (long)(Cm / 32) * (kg == 2 ? 1 : Cout / 256);
    const long per = (long)Cout * 9 * Cm;
    long sp = std::max<long>(1, std::min<long>(256 / std::max<long>(1, out_tiles), ntiles / 4));
    sp = std::min<long>(sp, std::min<long>(ws_floats, 16L << 20) / (per * kg));     // partial slices: at most 64 MB written + folded
    if (sp < 1 || ntiles < 8) return false;
    p->tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, p->tps);
    p->ntiles = ntiles;
    p->kg = kg;
    p->slices = p->splits * kg;
    p->need = (long)p->slices * per;
    return true;
}
template <int KG>
const char* w9s2_tag() { return __PRETTY_FUNCTION__; }
static void launch_w9s2(const float* dy, const float* x, float* ws, int N, int Cx, int Cm, int H, int W, int Cout,
                        const W9S2Plan& p, const JpCall& st) {
    const int dyb = (int)((long)N * Cout * (H / 2) * (W / 2) * 4), xb = (int)((long)N * Cx * H * W * 4);
    const float* gam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * (H / 2) * (W / 2), st) : nullptr;
    const float* xam = JP_NS == 2 ? jp_amax_of(x, (long)N * Cx * H * W, st) : nullptr;
    const double fl = JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * (H / 2) * (W / 2);
    if (p.kg == 2) {
        jp_prof_before(w9s2_tag<2>(), fl, st);
        hipLaunchKernelGGL((jp_wgrad_w9s2_kernel<2>), dim3(Cm / 32, 1, p.splits), dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                           p.ntiles, p.tps, dyb, xb, gam, xam);
    } else {
        jp_prof_before(w9s2_tag<1>(), fl, st);
        hipLaunchKernelGGL((jp_wgrad_w9s2_kernel<1>), dim3(Cm / 32, Cout / 256, p.splits), dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm,
                           H, W, p.ntiles, p.tps, dyb, xb, gam, xam);
    }
    jp_prof_after(st);
}
template <int MW, int KG, bool REFLECT>
const char* w9_tag() { return __PRETTY_FUNCTION__; }
template <int TR, bool REFLECT, int KG, int NCB = 2>
const char* w9s_tag() { return __PRETTY_FUNCTION__; }
template <bool REFLECT>
static void launch_w9(const float* dy, const float* x, float* ws, int N, int Cx, int Cm, int H, int W, int Cout,
                      const W9Plan& p, const JpCall& st) {
    if (p.split_mfma) {
        // executed FLOPs: 6 bf16 MFMA products per fp32 product
        const int dyb = (int)((long)N * Cout * H * W * 4);
        const int xb = (int)std::min<long>((long)N * Cx * H * W * 4, 0x7fffffffL);       // (w9_plan: the X tensor is < 2 GiB too)
        const float* gam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * H * W, st) : nullptr;
        const float* xam = JP_NS == 2 ? jp_amax_of(x, (long)N * Cx * H * W, st) : nullptr;
        if (p.narrow) {
            jp_prof_before(w9s_tag<W9S_TRN, REFLECT, 2>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
            dim3 grid(Cm / 64, jp_cdiv(Cout, 64), p.splits);
            hipLaunchKernelGGL((jp_wgrad_w9s_kernel<W9S_TRN, REFLECT, 2>), grid, dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                               p.ntiles, p.tps, dyb, xb, gam, xam);
        } else if (p.ncb1) {
            dim3 grid(Cm / 32, Cout / 256, p.splits);
            if (p.tr == 4) {
                jp_prof_before(w9s_tag<4, REFLECT, 1, 1>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
                hipLaunchKernelGGL((jp_wgrad_w9s_kernel<4, REFLECT, 1, 1>), grid, dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                                   p.ntiles, p.tps, dyb, xb, gam, xam);
            } else {
                jp_prof_before(w9s_tag<W9S_TR, REFLECT, 1, 1>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
                hipLaunchKernelGGL((jp_wgrad_w9s_kernel<W9S_TR, REFLECT, 1, 1>), grid, dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                                   p.ntiles, p.tps, dyb, xb, gam, xam);
            }
        } else {
            jp_prof_before(w9s_tag<W9S_TR, REFLECT, 1>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
            dim3 grid(Cm / 64, jp_cdiv(Cout, 128), p.splits);
            hipLaunchKernelGGL((jp_wgrad_w9s_kernel<W9S_TR, REFLECT, 1>), grid, dim3(512), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                               p.ntiles, p.tps, dyb, xb, gam, xam);
        }
        jp_prof_after(st);
        return;
    }
    jp_prof_before(p.narrow ? w9_tag<1, 2, REFLECT>() : w9_tag<2, 1, REFLECT>(), 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
    const int dyb = (int)((long)N * Cout * H * W * 4);          // < 2^31 (w9_plan): dY is addressed through a buffer resource
    if (p.narrow) {
        dim3 grid(Cm / 64, jp_cdiv(Cout, 64), p.splits);
        hipLaunchKernelGGL((jp_wgrad_w9_kernel<1, 2, 2, REFLECT>), grid, dim3(768), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                           p.ntiles, p.tps, dyb);
    } else {
        dim3 grid(Cm / 64, jp_cdiv(Cout, 128), p.splits);
        hipLaunchKernelGGL((jp_wgrad_w9_kernel<2, 2, 1, REFLECT>), grid, dim3(768), 0, st, dy, x, ws, Cout, Cx, Cm, H, W,
                           p.ntiles, p.tps, dyb);
    }
    jp_prof_after(st);
}

// ---- W7 stem wgrad (igemm_w7.h): 7x7 stride 2 pad 3, 3 or 6 input channels -> 64
struct W7Plan { int splits, tps, ntiles, slices; long need; };
static inline bool w7_plan(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad, long ws_floats, W7Plan* p) {
    if (!w9_enabled() || KH != 7 || stride != 2 || pad != 3 || (Cin != 3 && Cin != 6) || Cout != 64 || H % 2 || W % 2 ||
        (W / 2) % 32 || (H / 2) % 4 || (long)N * 64 * (H / 2) * (W / 2) * 4 >= (1L << 31) || (long)N * Cin * H * W >= (1L << 31))
        return false;
    const int ntiles = N * (H / 8) * (W / 64), kg = Cin == 3 ? 2 : 1, np = (49 * Cin + 31) / 32 * 32;
    long sp = std::max<long>(1, std::min<long>(512, ntiles / 4));
    sp = std::min<long>(sp, ws_floats / (64L * np * kg));
    if (sp < 1 || ntiles < 16) return false;
    p->tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, p->tps);
    p->ntiles = ntiles;
    p->slices = p->splits * kg;
    p->need = (long)p->slices * 64 * np;
    return true;
}
template <int CIN>
const char* w7_tag() { return __PRETTY_FUNCTION__; }
template <int CIN>
static void launch_w7(const float* dy, const float* x, float* dw, float* ws, int N, int H, int W, const W7Plan& p,
                      const JpCall& st) {
    jp_prof_before(w7_tag<CIN>(), 2.0 * 64 * 49.0 * CIN * (double)N * (H / 2) * (W / 2), st);
    hipLaunchKernelGGL((jp_wgrad_w7_kernel<CIN>), dim3(p.splits), dim3(640), 0, st, dy, x, ws, H, W, p.ntiles, p.tps,
                       (int)((long)N * 64 * (H / 2) * (W / 2) * 4));
    jp_prof_after(st);
    constexpr int NP = (49 * CIN + 31) / 32 * 32;
    hipLaunchKernelGGL((w7_reduce_kernel<CIN>), dim3(64 * NP / 64), dim3(1024), 0, st, ws, dw, p.slices);
}

// ---- W1 (igemm_w9.h): 1x1 stride-1 wgrad, single full-resolution source, 128-aligned input channels
struct W1Plan { int splits, tps, ntiles; long need; };
static inline bool w1_plan(int N, int Cm, int H, int W, int Cout, int KH, int stride, int pad, long ws_floats, W1Plan* p) {
    static const bool on = [] { const char* e = getenv("JP_W1"); return !(e && e[0] == '0'); }();
    if (!on || !w9_enabled() || KH != 1 || stride != 1 || pad != 0 || W % 32 || H % 4 || Cm < 128 || Cm % 128 || Cout < 192 ||
        (long)N * Cout * H * W * 4 >= (1L << 31))
        return false;
    const int ntiles = N * (H / 4) * (W / 32);
    const long out_tiles = (long)(Cm / 128) * jp_cdiv(Cout, 256), per = (long)Cout * Cm;
    static const long wgs = [] { const char* e = getenv("JP_W1_WGS"); return e ? atol(e) : 256L; }();
    long sp = std::max<long>(1, std::min<long>(wgs / std::max<long>(1, out_tiles), ntiles / 4));
    sp = std::min<long>(sp, ws_floats / per);
    if (sp < 1 || ntiles < 16) return false;
    p->tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, p->tps);
    p->ntiles = ntiles;
    p->need = (long)p->splits * per;
    return true;
}
static const char* w1_tag() { return "const char *w1_tag() [K = 1]"; }
static const char* w1s_tag() { return "const char *w1s_tag() [K = 1]"; }

}  // namespace

// wgrad of the (virtually concatenated) sources into the dw columns [dw_coff, dw_coff + c0+c1+c2) of a filter bank with
// dw_ctot input channels.  Sub-range calls (dw_coff > 0 or fewer channels than dw_ctot) must be single-source.
static int wgrad_impl(const float* x0, int c0, int up0, const float* x1, int c1, int up1, const float* x2, int c2, int up2,
                      const float* dy, float* dw, int N, int H, int W, int Cout, int KH, int stride, int pad,
                      int pad_mode, float* ws, long ws_floats, const JpCall& st, int dw_ctot, int dw_coff) {
    const int Cin = c0 + c1 + c2;
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const long npix = (long)N * OH * OW;
    JP_CHECK_ARG(npix < (1L << 31), "conv2d_wgrad: tensor too large");
    const int Kw = Cin * KH * KH;
    const bool whole = dw_coff == 0 && dw_ctot == Cin;
    if (whole && up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W)) {
        jp_up_head_wgrad(x0, dy, dw, N, c0, H / 2, W / 2, st, ws, ws_floats);
        JP_LAUNCH_CHECK();
    }
    if (whole && c1 == 0 && c2 == 0 && jp_c16_ok(c0, Cout, KH, stride, pad, pad_mode, H, W)) {
        jp_c16_wgrad(x0, up0, dy, dw, N, c0, Cout, H, W, st, ws, ws ? ws_floats : 0);
        JP_LAUNCH_CHECK();
    }
    if (whole && small_head(Cin, Cout, KH, stride, pad)) {
        jp_conv_small_wgrad(x0, c0, up0, x1, c1, up1, x2, c2, up2, dy, dw, N, H, W, Cout, pad_mode == JP_PAD_REFLECT, st, ws,
                            ws ? ws_floats : 0);
        JP_LAUNCH_CHECK();
    }
    WgradA a{dy, Cout, (int)npix, OH * OW};
    const Src3 src = make_src(x0, c0, up0, x1, c1, up1, x2, c2, up2, H, W);
    if (!ws) ws_floats = 0;
    // scalar-base loaders: K = (image, pixel padded to a multiple of 32) so a K chunk never straddles two images
    const int Ppad = pad32(OH * OW);
    const long kext = (long)N * Ppad;
    auto plan = [&](int Np, int* splits, int* kps, int per_cu = 2) {   // atomic-epilogue paths
        const bool narrow = Cout <= 64;
        const WgradPlan p = wgrad_plan(Cout, Np, npix, narrow ? 64 : 128, narrow ? 256 : 128, per_cu, 0);
        *splits = p.splits;
        *kps = p.kps;
    };
    // scalar-base paths: scratch-reduced split-K when the caller provided scratch and the plan prefers it
    auto go = [&](auto wm, auto wn, auto a_, auto b_, const WgradEpiT& e, int Np) {
        constexpr int WM = decltype(wm)::value, WN = decltype(wn)::value;
        const WgradPlan p = wgrad_plan(Cout, Np, kext, 64 * WM, 64 * WN, 3, ws_floats);
        if (p.use_ws) {
            WgradEpiWS ew{ws, Cout, Np};
            launch<true, WM, WN>(a_, b_, ew, Cout, Np, (int)kext, p.splits, p.kps, st);
            const long total = (long)Cout * Np;
            if (p.splits >= 32 && total <= (1L << 16))
                hipLaunchKernelGGL(wgrad_reduce_wide_kernel, dim3((int)((total + 63) / 64)), dim3(1024), 0, st, ws, dw, Cout,
                                   Np, p.splits, e.Cp, e.Cin, e.KHW, e.c_off, e.Ctot);
            else
                hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st,
                                   ws, dw, Cout, Np, p.splits, e.Cp, e.Cin, e.KHW, e.c_off, e.Ctot);
        } else {
            launch<true, WM, WN>(a_, b_, e, Cout, Np, (int)kext, p.splits, p.kps, st);
        }
    };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    const bool single = (c1 == 0 && c2 == 0 && up0 == 0 && (long)Cin * H * W < (1L << 31));
    int splits, kps;
    // table path over a channel sub-range [cb, cb+cn) of a single full-resolution source
    auto run_table = [&](int cb, int cn) -> int {
        const int Cp = cn, Np = KH * KH * Cp;    // the slot tables need no channel padding
        const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)Cp) + 1u;
        plan(Np, &splits, &kps);
        WgradEpiT e{dw, Cp, cn, KH * KH, dw_coff + cb, dw_ctot, magic};
        // split-K partial tiles through the caller's scratch when it is large enough (fixed-order fold: bit-reproducible); the
        // atomic epilogue otherwise.  (The scratch is free again here: a main pass that used it has been folded on this stream.)
        const bool via_ws = splits > 1 && ws && (long)splits * Cout * Np <= ws_floats;
        JP_KH_SWITCH(KH, {
            WgradBT1<KH_> b{x0 + (size_t)cb * H * W, Np, Cp, cn, Cin, H, W, (int)npix, OH, OW, stride, pad,
                            pad_mode == JP_PAD_REFLECT, magic};
            if (via_ws) {
                WgradEpiWS ew{ws, Cout, Np};
                launch_auto<true>(a, b, ew, Cout, Np, (int)npix, splits, kps, st);
            } else {
                launch_auto<true>(a, b, e, Cout, Np, (int)npix, splits, kps, st);
            }
        });
        if (via_ws) {
            const long total = (long)Cout * Np;
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, ws, dw, Cout,
                               Np, splits, e.Cp, e.Cin, e.KHW, e.c_off, e.Ctot);
        }
        return 0;
    };
    JP_CHECK_ARG(whole || single, "conv2d_wgrad: internal sub-range call must be single-source");
    W1Plan w1;
    if (single && ws && w1_plan(N, Cin, H, W, Cout, KH, stride, pad, ws_floats, &w1)) {
        if (w9s_enabled()) {    // W1S: the same tile and split-K plan on the bf16 pipe (igemm_w9s.h)
            const float* gam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * H * W, st) : nullptr;
            const float* xam = JP_NS == 2 ? jp_amax_of(x0, (long)N * Cin * H * W, st) : nullptr;
            jp_prof_before(w1s_tag(), JP_NPROD * 2.0 * Cout * (double)Cin * N * H * W, st);
            hipLaunchKernelGGL(jp_wgrad_w1s_kernel, dim3(Cin / 128, jp_cdiv(Cout, 256), w1.splits), dim3(512), 0, st, dy, x0, ws, Cout,
                               Cin, Cin, H, W, w1.ntiles, w1.tps, (int)((long)N * Cout * H * W * 4), gam, xam);
        } else {
            jp_prof_before(w1_tag(), 2.0 * Cout * (double)Cin * N * H * W, st);
            hipLaunchKernelGGL(jp_wgrad_w1_kernel, dim3(Cin / 128, jp_cdiv(Cout, 256), w1.splits), dim3(512), 0, st, dy, x0, ws, Cout,
                               Cin, Cin, H, W, w1.ntiles, w1.tps, (int)((long)N * Cout * H * W * 4));
        }
        jp_prof_after(st);
        const long total = (long)Cout * Cin;
        const int nblk = (int)((total / 4 + 63) / 64);
        if (w1.splits >= 64 && nblk < 2048)
            hipLaunchKernelGGL(wgrad_reduce4_kernel<8>, dim3(nblk), dim3(512), 0, st, ws, dw, Cout, Cin, w1.splits, Cin, 1, dw_coff,
                               dw_ctot);
        else
            hipLaunchKernelGGL(wgrad_reduce4_kernel<1>, dim3(nblk), dim3(64), 0, st, ws, dw, Cout, Cin, w1.splits, Cin, 1, dw_coff,
                               dw_ctot);
        JP_LAUNCH_CHECK();
    }
    W7Plan w7;
    if (single && whole && ws && w7_plan(N, Cin, H, W, Cout, KH, stride, pad, ws_floats, &w7)) {
        if (Cin == 3) launch_w7<3>(dy, x0, dw, ws, N, H, W, w7, st);
        else launch_w7<6>(dy, x0, dw, ws, N, H, W, w7, st);
        JP_LAUNCH_CHECK();
    }
    W9S2Plan w92;
    if (single && whole && ws && w9s2_plan(N, Cin, H, W, Cout, KH, stride, pad, pad_mode, ws_floats, &w92)) {
        launch_w9s2(dy, x0, ws, N, Cin, Cin, H, W, Cout, w92, st);
        const long total = (long)Cout * 9 * Cin;
        const int nblk = (int)((total / 4 + 63) / 64);
        if (w92.slices >= 64 && nblk < 2048)
            hipLaunchKernelGGL(wgrad_reduce4_kernel<8>, dim3(nblk), dim3(512), 0, st, ws, dw, Cout, 9 * Cin, w92.slices, Cin, 9,
                               dw_coff, dw_ctot);
        else
            hipLaunchKernelGGL(wgrad_reduce4_kernel<1>, dim3(nblk), dim3(64), 0, st, ws, dw, Cout, 9 * Cin, w92.slices, Cin, 9,
                               dw_coff, dw_ctot);
        JP_LAUNCH_CHECK();
    }
    W9Plan w9;
    // W9 patch kernel on the 64-aligned channels (+ a table pass for a short channel tail, e.g. 513 = 512 + 1): input patch
    // staged once per pixel tile for all 9 taps, dY fragments straight from global memory
    const int c9 = Cin / 64 * 64, tail9 = Cin - c9;
    if (single && ws && (tail9 == 0 || (tail9 <= 32 && c9 >= 128)) && (long)N * Cin * H * W * 4 < (1L << 31) &&
        w9_plan(N, c9, H, W, Cout, KH, stride, pad, ws_floats, &w9)) {
        if (pad_mode == JP_PAD_REFLECT) launch_w9<true>(dy, x0, ws, N, Cin, c9, H, W, Cout, w9, st);
        else launch_w9<false>(dy, x0, ws, N, Cin, c9, H, W, Cout, w9, st);
        const long total = (long)Cout * 9 * c9;
        const int nblk = (int)((total / 4 + 63) / 64);
        if (w9.slices >= 64 && nblk < 2048)          // few outputs, many slices: 8 slice lanes per output quad
            hipLaunchKernelGGL(wgrad_reduce4_kernel<8>, dim3(nblk), dim3(512), 0, st, ws, dw, Cout, 9 * c9, w9.slices, c9, 9,
                               dw_coff, dw_ctot);
        else
            hipLaunchKernelGGL(wgrad_reduce4_kernel<1>, dim3(nblk), dim3(64), 0, st, ws, dw, Cout, 9 * c9, w9.slices, c9, 9,
                               dw_coff, dw_ctot);
        if (tail9) {
            const int rc = run_table(c9, tail9);
            if (rc) return rc;
        }
    } else
    if (!single && Cin < 32) {          // generic (channel-major) path: multi-source inputs with few channels
        WgradEpi e{dw, Kw};
        plan(Kw, &splits, &kps);
        JP_KH_SWITCH(KH, {
            WgradB<KH_> b{src, Kw, (int)npix, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
            launch_auto<true>(a, b, e, Cout, Kw, (int)npix, splits, kps, st);
        });
    } else if (!whole && Cin < 16) {    // a few channels of a wider filter bank (the disparity channel of the iconv input)
        const int rc = run_table(0, Cin);
        if (rc) return rc;
    } else if (single && Cout > 64 && Cin >= 128 && (Cin % 128 == 0 || Cin % 128 <= 32)) {
        // uniform-tap path on the 128-aligned part (+ a table pass for a short channel tail, e.g. 513 = 512 + 1)
        const int Cm = Cin / 128 * 128, tail = Cin - Cm;
        const int Np = KH * KH * Cm;
        const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)Cm) + 1u;
        const bool scalar_ok = Cout % 8 == 0 && (long)8 * H * W * 4 < (1L << 31);
        WgradEpiT e{dw, Cm, Cm, KH * KH, dw_coff, dw_ctot, magic};
        if (scalar_ok) {   // scalar-base loaders
            WgradAS as{dy, Cout, (int)kext, OH * OW, Ppad};
            JP_KH_SWITCH(KH, {
                if (pad_mode == JP_PAD_REFLECT) {
                    WgradBUS<KH_, true> b{x0, Cm, Cin, H, W, OH, OW, stride, pad, Ppad};
                    go(I2{}, I2{}, as, b, e, Np);
                } else {
                    WgradBUS<KH_, false> b{x0, Cm, Cin, H, W, OH, OW, stride, pad, Ppad};
                    go(I2{}, I2{}, as, b, e, Np);
                }
            });
        } else {
            plan(Np, &splits, &kps);
            JP_KH_SWITCH(KH, {
                WgradBU<KH_> b{x0, Cm, Cm, Cin, H, W, (int)npix, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT};
                launch<true, 2, 2>(a, b, e, Cout, Np, (int)npix, splits, kps, st);
            });
        }
        if (tail) {
            const int rc = run_table(Cm, tail);
            if (rc) return rc;
        }
    } else if (single && (Cin == 64 || ((Cin == 16 || Cin == 32) && Cout <= 64)) && Cout % 8 == 0 &&
               (long)8 * H * W * 4 < (1L << 31)) {
        // 16 / 32 / 64 input channels (ResNet stem + layer1, BEV decoder): whole taps per N tile, scalar-base loaders
        const int Np = KH * KH * Cin;
        const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)Cin) + 1u;
        WgradEpiT e{dw, Cin, Cin, KH * KH, dw_coff, dw_ctot, magic};
        WgradAS as{dy, Cout, (int)kext, OH * OW, Ppad};
#define JP_BMS(REFL, WMv, WNv, TPTv, CPTv)                                              \
    {                                                                                   \
        WgradBMS<KH_, REFL, TPTv, CPTv> b{x0, Cin, H, W, OH, OW, stride, pad, Ppad};    \
        go(std::integral_constant<int, WMv>{}, std::integral_constant<int, WNv>{}, as, b, e, Np); \
    }
        JP_KH_SWITCH(KH, {
            if (pad_mode == JP_PAD_REFLECT) {
                if (Cin == 16) JP_BMS(true, 1, 4, 16, 16)
                else if (Cin == 32) JP_BMS(true, 1, 4, 8, 32)
                else if (Cout <= 64) JP_BMS(true, 1, 4, 4, 64)
                else JP_BMS(true, 2, 2, 2, 64)
            } else {
                if (Cin == 16) JP_BMS(false, 1, 4, 16, 16)
                else if (Cin == 32) JP_BMS(false, 1, 4, 8, 32)
                else if (Cout <= 64) JP_BMS(false, 1, 4, 4, 64)
                else JP_BMS(false, 2, 2, 2, 64)
            }
        });
#undef JP_BMS
    } else if (single) {
        const int rc = run_table(0, Cin);
        if (rc) return rc;
    } else {
        const int Cp = pad32(Cin), Np = KH * KH * Cp;
        const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)Cp) + 1u;
        plan(Np, &splits, &kps);
        WgradEpiT e{dw, Cp, Cin, KH * KH, 0, Cin, magic};
        JP_KH_SWITCH(KH, {
            WgradBT<KH_> b{src, Np, Cp, Cin, (int)npix, OH, OW, stride, pad, pad_mode == JP_PAD_REFLECT, magic};
            launch_auto<true>(a, b, e, Cout, Np, (int)npix, splits, kps, st);
        });
    }
    JP_LAUNCH_CHECK();
}


// ---- W4S (igemm_w4s.h): split-bf16 parity-class wgrad of the upsampled iconv segment; JP_W9S=0 keeps the generic
// WgradAP/WgradBP instantiation.  Same partial-sum layout ws[split][co][16*Cx], folded by wgrad_fold_parity_kernel.
constexpr int W4S_TR = 2;
struct W4SPlan { int splits, tps, ntiles; long need; };
static inline bool w4s_plan(int N, int Cx, int h2, int w2, int Cout, long ws_floats, W4SPlan* p) {
    if (!w9s_enabled() || Cx % 64 || w2 % 32 || h2 % W4S_TR || (long)N * Cout * h2 * w2 * 16 >= (1L << 31)) return false;
    const int ntiles = N * (h2 / W4S_TR) * (w2 / 32);
    const long out_tiles = 2L * (Cx / 64) * jp_cdiv(Cout, 128), per = (long)Cout * 16 * Cx;
    long sp = std::max<long>(1, std::min<long>(jp_cdiv(256, out_tiles), ntiles / 2));
    sp = std::min<long>(sp, ws_floats / per);
    if (sp < 1 || ntiles < 8) return false;
    p->tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, p->tps);
    p->ntiles = ntiles;
    p->need = (long)p->splits * per;
    return true;
}
template <int TR>
const char* w4s_tag() { return __PRETTY_FUNCTION__; }

// one channel segment is eligible for the per-segment wgrad (no materialised concat): full-resolution segments run the
// single-source paths on their own tensor, the upsampled one the parity-class kernels
static bool wgrad_segments_ok(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W, int Cout, int KH,
                              int stride, int pad, int pad_mode) {
    const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2};
    int nseg = 0, nup = 0;
    for (int i = 0; i < 3; ++i) {
        if (!cs[i]) continue;
        ++nseg;
        if (us[i]) {
            ++nup;
            if (cs[i] % 128 || Cout % 8 || Cout <= 64) return false;
        }
    }
    if (nseg < 2 || nup != 1) return false;
    return KH == 3 && stride == 1 && pad == 1 && pad_mode == JP_PAD_REFLECT && H % 2 == 0 && (W / 2) % 32 == 0 && W % 2 == 0 &&
           (long)N * H * W < (1L << 31);
}

extern "C" int jp_conv2d_wgrad_src3(const float* x0, int c0, int up0, const float* x1, int c1, int up1,
                                    const float* x2, int c2, int up2, const float* dy, float* dw, int N, int H, int W,
                                    int Cout, int KH, int stride, int pad, int pad_mode, int accumulate,
                                    float* ws, long ws_floats, const float* amax_x0, const float* amax_x1, const float* amax_x2,
                                    const float* amax_dy, float* amax_ws, void* stream) {
    JP_CHECK_ARG(x0 && dy && dw, "conv2d_wgrad: null pointer");
    JP_CHECK_ARG(JP_NS != 2 || amax_ws || (amax_dy && amax_x0 && (!c1 || amax_x1) && (!c2 || amax_x2)),
                 "conv2d_wgrad"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(x0, amax_x0);
    ax.know(x1, amax_x1);
    ax.know(x2, amax_x2);
    ax.know(dy, amax_dy);
    ax.ws = amax_ws;
    const JpCall st((hipStream_t)stream, &ax);
    const int Cin = c0 + c1 + c2;
    if (!accumulate) JP_HIP(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)Cout * Cin * KH * KH, st));
    if (ws && wgrad_segments_ok(c0, up0, c1, up1, c2, up2, N, H, W, Cout, KH, stride, pad, pad_mode)) {
        const float* xs[3] = {x0, x1, x2};
        const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2};
        int coff = 0;
        for (int i = 0; i < 3; ++i) {
            if (!cs[i]) continue;
            if (!us[i]) {
                const int rc = wgrad_impl(xs[i], cs[i], 0, nullptr, 0, 0, nullptr, 0, 0, dy, dw, N, H, W, Cout, KH, stride, pad,
                                          pad_mode, ws, ws_floats, st, Cin, coff);
                if (rc) return rc;
            } else {
                const int h2 = H / 2, w2 = W / 2, Cx = cs[i], Np = 16 * Cx;
                const long Ncl = (long)N * h2 * w2;
                W4SPlan q;
                if (w4s_plan(N, Cx, h2, w2, Cout, ws_floats, &q)) {
                    // executed FLOPs: 6 bf16 MFMA products per fp32 product, 16 (class, slot) GEMMs over the half-res pixels
                    const float* gam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * H * W, st) : nullptr;
                    const float* xam = JP_NS == 2 ? jp_amax_of(xs[i], (long)N * Cx * h2 * w2, st) : nullptr;
                    jp_prof_before(w4s_tag<W4S_TR>(), JP_NPROD * 2.0 * Cout * 16.0 * Cx * (double)Ncl, st);
                    hipLaunchKernelGGL((jp_wgrad_w4s_kernel<W4S_TR>), dim3(Cx / 64, jp_cdiv(Cout, 128), 2 * q.splits), dim3(512), 0,
                                       st, dy, xs[i], ws, Cout, Cx, h2, w2, q.ntiles, q.tps, (int)((long)N * Cout * H * W * 4), gam, xam);
                    jp_prof_after(st);
                    const long total = (long)Cout * Cx * 9;
                    hipLaunchKernelGGL(wgrad_fold_parity_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0,
                                       st, ws, dw, Cout, Cx, q.splits, coff, Cin);
                    coff += cs[i];
                    continue;
                }
                WgradPlan p = wgrad_plan(Cout, Np, Ncl, 128, 128, 3, ws_floats);
                if (!p.use_ws) {    // this path always reduces through scratch: take the largest split that fits
                    long sp = std::max<long>(1, std::min<long>(ws_floats / ((long)Cout * Np), jp_cdiv(Ncl, KC) / 4));
                    JP_CHECK_ARG(ws_floats >= (long)Cout * Np, "conv2d_wgrad: scratch too small (jp_conv2d_wgrad_src3_ws_floats)");
                    sp = std::min<long>(sp, 64);
                    p.kps = (int)(jp_cdiv(jp_cdiv(Ncl, KC), sp) * KC);
                    p.splits = jp_cdiv(Ncl, p.kps);
                }
                WgradAP a{dy, Cout, h2, w2, 4 * Cx};
                WgradBP b{xs[i], Cx, h2, w2};
                WgradEpiWS ew{ws, Cout, Np};
                launch<true, 2, 2>(a, b, ew, Cout, Np, (int)Ncl, p.splits, p.kps, st);
                const long total = (long)Cout * Cx * 9;
                hipLaunchKernelGGL(wgrad_fold_parity_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st,
                                   ws, dw, Cout, Cx, p.splits, coff, Cin);
            }
            coff += cs[i];
        }
        JP_LAUNCH_CHECK();
    }
    return wgrad_impl(x0, c0, up0, x1, c1, up1, x2, c2, up2, dy, dw, N, H, W, Cout, KH, stride, pad, pad_mode, ws, ws_floats, st,
                      Cin, 0);
}

// scratch floats for jp_conv2d_wgrad_src3 on a multi-source input (0 = use the single-source query / no benefit)
extern "C" long jp_conv2d_wgrad_src3_ws_floats(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W,
                                               int Cout, int KH, int stride, int pad, int pad_mode) {
    if (c1 == 0 && c2 == 0 && jp_c16_ok(c0, Cout, KH, stride, pad, pad_mode, H, W)) return jp_c16_wgrad_ws_floats(N, c0, Cout, H, W);
    // disparity head on an upsampled source: the gathered dY sums + the workgroups' partial sums (fixed-order fold)
    if (up_head(c0, up0, c1, c2, Cout, KH, stride, pad, pad_mode, H, W)) return jp_up_head_wgrad_ws_floats(N, c0, H / 2, W / 2);
    if (small_head(c0 + c1 + c2, Cout, KH, stride, pad))
        return jp_conv_small_wgrad_ws_floats(N, c0 + c1 + c2, H, W, Cout, c1 == 0 && c2 == 0 && !up0);
    if (!wgrad_segments_ok(c0, up0, c1, up1, c2, up2, N, H, W, Cout, KH, stride, pad, pad_mode)) return 0;
    const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2};
    const long cap = 48L << 20;
    long need = 0;
    for (int i = 0; i < 3; ++i) {
        if (!cs[i]) continue;
        if (us[i]) {
            const WgradPlan p = wgrad_plan(Cout, 16 * cs[i], (long)N * (H / 2) * (W / 2), 128, 128, 3, cap);
            need = std::max(need, p.use_ws ? p.ws_need : (long)Cout * 16 * cs[i]);
            W4SPlan q;
            if (w4s_plan(N, cs[i], H / 2, W / 2, Cout, cap, &q)) need = std::max(need, q.need);
        } else if (cs[i] >= 16) {
            const int Np = KH * KH * (cs[i] >= 64 ? cs[i] / 64 * 64 : cs[i]);
            const WgradPlan p = wgrad_plan(Cout, Np, (long)N * H * W, 128, 128, 3, cap);
            if (p.use_ws) need = std::max(need, p.ws_need);
        }
    }
    return need;
}

extern "C" int jp_conv2d_wgrad(const float* x, const float* dy, float* dw, int N, int Cin, int H, int W, int Cout,
                               int KH, int stride, int pad, int pad_mode, int accumulate, float* ws, long ws_floats,
                               const float* amax_x, const float* amax_dy, float* amax_ws, void* stream) {
    return jp_conv2d_wgrad_src3(x, Cin, 0, nullptr, 0, 0, nullptr, 0, 0, dy, dw, N, H, W, Cout, KH, stride, pad,
                                pad_mode, accumulate, ws, ws_floats, amax_x, nullptr, nullptr, amax_dy, amax_ws, stream);
}

// floats of optional caller scratch with which jp_conv2d_wgrad[_src3] merges its split-K partial tiles through a
// reduction pass instead of device-scope atomics (0 = no benefit for this shape).  Capped at 32 Mi floats.
extern "C" long jp_conv2d_wgrad_ws_floats(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad) {
    const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KH) / stride + 1;
    const long npix = (long)N * OH * OW, cap = 32L << 20;
    if (jp_c16_ok(Cin, Cout, KH, stride, pad, 0, H, W)) return jp_c16_wgrad_ws_floats(N, Cin, Cout, H, W);
    if (small_head(Cin, Cout, KH, stride, pad)) return jp_conv_small_wgrad_ws_floats(N, Cin, H, W, Cout, 1);
    W7Plan w7;
    if (w7_plan(N, Cin, H, W, Cout, KH, stride, pad, cap, &w7)) return w7.need;
    W1Plan w1;
    const long need1 = w1_plan(N, Cin, H, W, Cout, KH, stride, pad, cap, &w1) ? w1.need : 0;
    // the slot-table passes (odd channel counts, the 1-channel tail of the 513-channel iconv banks, Cout % 8 != 0): scratch for their
    // split-K partial tiles so that they are folded in a fixed order instead of meeting in atomics (round 6)
    auto table_need = [&](int cn) -> long {
        const int Npt = KH * KH * cn;
        const bool nrw = Cout <= 64;
        const WgradPlan pt = wgrad_plan(Cout, Npt, npix, nrw ? 64 : 128, nrw ? 256 : 128, 2, 0);
        const long n = (long)pt.splits * Cout * Npt;
        return (pt.splits > 1 && n <= cap) ? n : 0;
    };
    const int tail_c = (Cout > 64 && Cin >= 128 && Cin % 128 != 0 && Cin % 128 <= 32) ? Cin % 128 : 0;
    const long need_t = tail_c ? table_need(tail_c) : table_need(Cin);
    if (Cout % 8 != 0 || Cin < 16) return need_t;
    const int Np = KH * KH * (Cin >= 64 ? Cin / 64 * 64 : Cin);
    const bool narrow = Cout <= 64 && Cin <= 64;
    const WgradPlan p = wgrad_plan(Cout, Np, (long)N * pad32(OH * OW), narrow ? 64 : 128, narrow ? 256 : 128, 3, cap);
    W9Plan w9;
    const long need9 = w9_plan(N, Cin / 64 * 64, H, W, Cout, KH, stride, pad, cap, &w9) ? w9.need : 0;
    W9S2Plan w92;
    const long need92 = w9s2_plan(N, Cin, H, W, Cout, KH, stride, pad, 0, cap, &w92) ? w92.need : 0;
    return std::max(std::max(std::max(std::max(p.use_ws ? p.ws_need : 0, need9), need1), need92), need_t);
}
