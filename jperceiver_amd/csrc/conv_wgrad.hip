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

// ---- geometry of one weight-gradient call, read by every plan predicate and launcher (the scratch queries: null pointers).  The
// (virtually concatenated) sources fill the dw columns [dw_coff, dw_coff + Cin()) of a filter bank with dw_ctot input channels.
struct WgradGeom {
    struct Src { const float* p; int c, up; } s[3];
    const float* dy;
    float* dw;
    int N, H, W, Cout, KH, stride, pad, pad_mode, OH, OW;
    long npix;
    int dw_ctot, dw_coff;
    int Cin() const { return s[0].c + s[1].c + s[2].c; }
    int KK() const { return KH * KH; }
    bool reflect() const { return pad_mode == JP_PAD_REFLECT; }
    bool whole() const { return dw_coff == 0 && dw_ctot == Cin(); }
    bool one() const { return s[1].c == 0 && s[2].c == 0; }
    bool single() const { return one() && s[0].up == 0 && (long)Cin() * H * W < (1L << 31); }      // one full-resolution tensor
    // scalar-base loaders: K = (image, pixel padded to a multiple of 32) so a K chunk never straddles two images
    int Ppad() const { return pad32(OH * OW); }
    long kext() const { return (long)N * Ppad(); }
};
static WgradGeom wgrad_geom(WgradGeom::Src s0, WgradGeom::Src s1, WgradGeom::Src s2, const float* dy, float* dw, int N, int H, int W,
                            int Cout, int KH, int stride, int pad, int pad_mode) {
    WgradGeom g{{s0, s1, s2}, dy, dw, N, H, W, Cout, KH, stride, pad, pad_mode};
    g.OH = (H + 2 * pad - KH) / stride + 1;
    g.OW = (W + 2 * pad - KH) / stride + 1;
    g.npix = (long)N * g.OH * g.OW;
    g.dw_ctot = g.Cin();
    g.dw_coff = 0;
    return g;
}
// source i of g as a call of its own that fills its own columns (from coff on) of g's filter bank
static WgradGeom wgrad_segment(WgradGeom q, int i, int coff) {
    q.s[0] = q.s[i];
    q.s[1] = q.s[2] = WgradGeom::Src{nullptr, 0, 0};
    q.dw_coff = coff;
    return q;
}

// ---- what the launch side and the scratch queries both read.  Channels the aligned kernels cover (W9: multiples of 64; uniform-tap:
// multiples of 128, the same number under uniform_tap_ok; BMS: all 16 / 32 / 64); a table pass takes the rest
static inline int wgrad_aligned(int Cin) { return Cin >= 64 ? Cin / 64 * 64 : Cin; }
// uniform-tap route: a 128-aligned part plus a short channel tail (e.g. 513 = 512 + 1)
static inline bool uniform_tap_ok(int Cin, int Cout) { return Cout > 64 && Cin >= 128 && Cin % 128 <= 32; }
// atomic-epilogue passes of the generic engine, tile = launch_auto's: 64 x 256 up to 64 output channels, 128 x 128 above
static inline WgradPlan atomic_plan(const WgradGeom& g, int Np) {
    const bool narrow = g.Cout <= 64;
    return wgrad_plan(g.Cout, Np, g.npix, narrow ? 64 : 128, narrow ? 256 : 128, 2, 0);
}
// slot-table pass over cn channels: the atomic plan, through the caller's scratch where that is large enough (fixed-order fold)
static inline WgradPlan table_plan(const WgradGeom& g, int cn, long ws_floats) {
    WgradPlan p = atomic_plan(g, g.KK() * cn);
    p.ws_need = (long)p.splits * g.Cout * g.KK() * cn;
    p.use_ws = p.splits > 1 && p.ws_need <= ws_floats;
    return p;
}
// scalar-base passes (uniform-tap, BMS): scratch-reduced split-K when scratch is there and the plan prefers it.  The 64 x 256 tile is
// BMS's for <= 64 output channels; uniform-tap has more than 64 of them and always runs 128 x 128.
static inline bool scalar_narrow(const WgradGeom& g) { return g.Cout <= 64 && g.Cin() <= 64; }
static inline WgradPlan scalar_plan(const WgradGeom& g, int Np, long ws_floats) {
    const bool narrow = scalar_narrow(g);
    return wgrad_plan(g.Cout, Np, g.kext(), narrow ? 64 : 128, narrow ? 256 : 128, 3, ws_floats);
}
// operand magnitudes of the split-bf16 kernels (scale.hip) on dY and on g's first source, dY first
struct WgradAmax { const float *g, *x; };
static inline WgradAmax wgrad_amax(const WgradGeom& g, const JpCall& st) {
    if (JP_NS != 2) return WgradAmax{nullptr, nullptr};
    const long nx = (long)g.N * g.s[0].c * (g.H >> g.s[0].up) * (g.W >> g.s[0].up);
    return WgradAmax{jp_amax_of(g.dy, (long)g.N * g.Cout * g.OH * g.OW, st), jp_amax_of(g.s[0].p, nx, st)};
}
// split of a slice kernel (W1, W7, W9, W9S2, W4S): ntiles pixel tiles over at most sp splits of kg K slices each, `per` floats of
// scratch a slice; refused below min_tiles tiles or where not even one split fits
struct SlicePlan { int splits, tps, ntiles, slices; long need; };
static inline bool slice_plan(SlicePlan* p, int ntiles, int min_tiles, long sp, int kg, long per) {
    if (sp < 1 || ntiles < min_tiles) return false;
    p->tps = (int)jp_cdiv(ntiles, sp);
    p->splits = jp_cdiv(ntiles, p->tps);
    p->ntiles = ntiles;
    p->slices = p->splits * kg;
    p->need = (long)p->slices * per;
    return true;
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
struct W9Plan : SlicePlan { int narrow, split_mfma, ncb1, tr; };
// W9S with 256 output x 32 input channels per workgroup (igemm_w9s.h NCB = 1) for layers whose output channels fill 256-row tiles;
// JP_W9S_NCB=2 keeps the 128 x 64 tiles of round 3
static inline bool w9s_ncb1(int Cout, int narrow) {
    static const bool on = [] { const char* e = getenv("JP_W9S_NCB"); return !(e && e[0] == '2'); }();
    return on && !narrow && Cout % 256 == 0;
}
// Cm: the 64-aligned channels the kernel covers (of g.Cin() in the tensor)
static inline bool w9_plan(const WgradGeom& g, int Cm, long ws_floats, W9Plan* p) {
    const int N = g.N, H = g.H, W = g.W, Cout = g.Cout;
    if (!w9_enabled() || g.KH != 3 || g.stride != 1 || g.pad != 1 || W % 32 || Cm < 64 || Cm % 64 || Cout < 48 ||
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
    const long sp = std::max<long>(1, std::min<long>(wgs / std::max<long>(1, out_tiles), ntiles / 2));
    p->narrow = narrow;
    return slice_plan(p, ntiles, 8, std::min<long>(sp, ws_floats / (per * kg)), kg, per);
}
// W9S2 (igemm_w9s2.h): the 3x3 stride-2 zero-pad weight gradient of the ResNet stage transitions on the bf16 pipe; JP_W9S2=0 (or
// JP_W9S=0) keeps the exact-fp32 generic engine.
struct W9S2Plan : SlicePlan { int kg; };
static inline bool w9s2_plan(const WgradGeom& g, long ws_floats, W9S2Plan* p) {
    const int N = g.N, Cm = g.Cin(), H = g.H, W = g.W, Cout = g.Cout;
    static const bool on = [] { const char* e = getenv("JP_W9S2"); return !(e && e[0] == '0'); }();
    if (!on || !w9s_enabled() || g.KH != 3 || g.stride != 2 || g.pad != 1 || g.reflect() || (H & 1) || (W & 1) ||
        (W / 2) % 32 || (H / 2) % 2 || Cm < 32 || Cm % 32 || !(Cout == 128 || Cout % 256 == 0) ||
        (long)N * Cout * (H / 2) * (W / 2) * 4 >= (1L << 31) || (long)N * Cm * H * W * 4 >= (1L << 31))
        return false;
    const int kg = Cout == 128 ? 2 : 1, ntiles = N * (H / 4) * (W / 64);
    const long out_tiles = (long)(Cm / 32) * (kg == 2 ? 1 : Cout / 256), per = (long)Cout * 9 * Cm;
    const long sp = std::max<long>(1, std::min<long>(256 / std::max<long>(1, out_tiles), ntiles / 4));
    p->kg = kg;
    return slice_plan(p, ntiles, 8, std::min<long>(sp, std::min<long>(ws_floats, 16L << 20) / (per * kg)), kg, per);  // at most 64 MB of slices
}
template <int KG>
const char* w9s2_tag() { return __PRETTY_FUNCTION__; }
template <int KG>
static void launch_w9s2(const WgradGeom& g, const W9S2Plan& p, float* ws, const JpCall& st) {
    const int N = g.N, Cm = g.Cin(), H = g.H, W = g.W, Cout = g.Cout;
    const int dyb = (int)((long)N * Cout * (H / 2) * (W / 2) * 4), xb = (int)((long)N * Cm * H * W * 4);
    const WgradAmax am = wgrad_amax(g, st);
    jp_prof_before(w9s2_tag<KG>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * (H / 2) * (W / 2), st);
    hipLaunchKernelGGL((jp_wgrad_w9s2_kernel<KG>), dim3(Cm / 32, KG == 2 ? 1 : Cout / 256, p.splits), dim3(512), 0, st, g.dy, g.s[0].p,
                       ws, Cout, Cm, Cm, H, W, p.ntiles, p.tps, dyb, xb, am.g, am.x);
    jp_prof_after(st);
}
template <int MW, int KG, bool REFLECT>
const char* w9_tag() { return __PRETTY_FUNCTION__; }
template <int TR, bool REFLECT, int KG, int NCB = 2>
const char* w9s_tag() { return __PRETTY_FUNCTION__; }
// executed FLOPs of the W9S kernels: JP_NPROD bf16 MFMA products per fp32 product
template <int TR, bool REFLECT, int KG, int NCB>
static void launch_w9s(dim3 grid, const WgradGeom& g, int Cm, const W9Plan& p, float* ws, const JpCall& st) {
    const int N = g.N, Cx = g.Cin(), H = g.H, W = g.W, Cout = g.Cout;
    const int dyb = (int)((long)N * Cout * H * W * 4);          // < 2^31 (w9_plan): dY is addressed through a buffer resource
    const int xb = (int)std::min<long>((long)N * Cx * H * W * 4, 0x7fffffffL);       // (the route: the X tensor is < 2 GiB too)
    const WgradAmax am = wgrad_amax(g, st);
    jp_prof_before(w9s_tag<TR, REFLECT, KG, NCB>(), JP_NPROD * 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
    hipLaunchKernelGGL((jp_wgrad_w9s_kernel<TR, REFLECT, KG, NCB>), grid, dim3(512), 0, st, g.dy, g.s[0].p, ws, Cout, Cx, Cm, H, W,
                       p.ntiles, p.tps, dyb, xb, am.g, am.x);
    jp_prof_after(st);
}
template <bool REFLECT>
static void launch_w9(const WgradGeom& g, int Cm, const W9Plan& p, float* ws, const JpCall& st) {
    const int N = g.N, Cx = g.Cin(), H = g.H, W = g.W, Cout = g.Cout, sp = p.splits;
    if (p.split_mfma) {
        if (p.narrow) launch_w9s<W9S_TRN, REFLECT, 2, 2>(dim3(Cm / 64, jp_cdiv(Cout, 64), sp), g, Cm, p, ws, st);
        else if (p.ncb1 && p.tr == 4) launch_w9s<4, REFLECT, 1, 1>(dim3(Cm / 32, Cout / 256, sp), g, Cm, p, ws, st);
        else if (p.ncb1) launch_w9s<W9S_TR, REFLECT, 1, 1>(dim3(Cm / 32, Cout / 256, sp), g, Cm, p, ws, st);
        else launch_w9s<W9S_TR, REFLECT, 1, 2>(dim3(Cm / 64, jp_cdiv(Cout, 128), sp), g, Cm, p, ws, st);
        return;
    }
    jp_prof_before(p.narrow ? w9_tag<1, 2, REFLECT>() : w9_tag<2, 1, REFLECT>(), 2.0 * Cout * 9.0 * Cm * (double)N * H * W, st);
    const int dyb = (int)((long)N * Cout * H * W * 4);
    const dim3 grid(Cm / 64, jp_cdiv(Cout, p.narrow ? 64 : 128), sp);
    hipLaunchKernelGGL((p.narrow ? jp_wgrad_w9_kernel<1, 2, 2, REFLECT> : jp_wgrad_w9_kernel<2, 2, 1, REFLECT>), grid, dim3(768), 0, st,
                       g.dy, g.s[0].p, ws, Cout, Cx, Cm, H, W, p.ntiles, p.tps, dyb);
    jp_prof_after(st);
}

// ---- W7 stem wgrad (igemm_w7.h): 7x7 stride 2 pad 3, 3 or 6 input channels -> 64
struct W7Plan : SlicePlan {};
static inline bool w7_plan(const WgradGeom& g, long ws_floats, W7Plan* p) {
    const int N = g.N, Cin = g.Cin(), H = g.H, W = g.W;
    if (!w9_enabled() || g.KH != 7 || g.stride != 2 || g.pad != 3 || (Cin != 3 && Cin != 6) || g.Cout != 64 || H % 2 || W % 2 ||
        (W / 2) % 32 || (H / 2) % 4 || (long)N * 64 * (H / 2) * (W / 2) * 4 >= (1L << 31) || (long)N * Cin * H * W >= (1L << 31))
        return false;
    const int ntiles = N * (H / 8) * (W / 64), kg = Cin == 3 ? 2 : 1, np = (49 * Cin + 31) / 32 * 32;
    const long sp = std::max<long>(1, std::min<long>(512, ntiles / 4));
    return slice_plan(p, ntiles, 16, std::min<long>(sp, ws_floats / (64L * np * kg)), kg, 64L * np);
}
template <int CIN>
const char* w7_tag() { return __PRETTY_FUNCTION__; }
template <int CIN>
static void launch_w7(const WgradGeom& g, const W7Plan& p, float* ws, const JpCall& st) {
    const int N = g.N, H = g.H, W = g.W;
    jp_prof_before(w7_tag<CIN>(), 2.0 * 64 * 49.0 * CIN * (double)N * (H / 2) * (W / 2), st);
    hipLaunchKernelGGL((jp_wgrad_w7_kernel<CIN>), dim3(p.splits), dim3(640), 0, st, g.dy, g.s[0].p, ws, H, W, p.ntiles, p.tps,
                       (int)((long)N * 64 * (H / 2) * (W / 2) * 4));
    jp_prof_after(st);
    constexpr int NP = (49 * CIN + 31) / 32 * 32;
    hipLaunchKernelGGL((w7_reduce_kernel<CIN>), dim3(64 * NP / 64), dim3(1024), 0, st, ws, g.dw, p.slices);
}

// ---- W1 (igemm_w9.h): 1x1 stride-1 wgrad, single full-resolution source, 128-aligned input channels
struct W1Plan : SlicePlan {};
static inline bool w1_plan(const WgradGeom& g, long ws_floats, W1Plan* p) {
    const int N = g.N, Cm = g.Cin(), H = g.H, W = g.W, Cout = g.Cout;
    static const bool on = [] { const char* e = getenv("JP_W1"); return !(e && e[0] == '0'); }();
    if (!on || !w9_enabled() || g.KH != 1 || g.stride != 1 || g.pad != 0 || W % 32 || H % 4 || Cm < 128 || Cm % 128 || Cout < 192 ||
        (long)N * Cout * H * W * 4 >= (1L << 31))
        return false;
    const int ntiles = N * (H / 4) * (W / 32);
    const long out_tiles = (long)(Cm / 128) * jp_cdiv(Cout, 256), per = (long)Cout * Cm;
    static const long wgs = [] { const char* e = getenv("JP_W1_WGS"); return e ? atol(e) : 256L; }();
    const long sp = std::max<long>(1, std::min<long>(wgs / std::max<long>(1, out_tiles), ntiles / 4));
    return slice_plan(p, ntiles, 16, std::min<long>(sp, ws_floats / per), 1, per);
}
static const char* w1_tag() { return "const char *w1_tag() [K = 1]"; }
static const char* w1s_tag() { return "const char *w1s_tag() [K = 1]"; }

}  // namespace

// ---- W4S (igemm_w4s.h): split-bf16 parity-class wgrad of the upsampled iconv segment; JP_W9S=0 keeps the generic
// WgradAP/WgradBP instantiation.  Same partial-sum layout ws[split][co][16*Cx], folded by wgrad_fold_parity_kernel.
constexpr int W4S_TR = 2;
struct W4SPlan : SlicePlan {};
static inline bool w4s_plan(const WgradGeom& q, long ws_floats, W4SPlan* p) {
    const int N = q.N, Cx = q.s[0].c, h2 = q.H / 2, w2 = q.W / 2, Cout = q.Cout;
    if (!w9s_enabled() || Cx % 64 || w2 % 32 || h2 % W4S_TR || (long)N * Cout * h2 * w2 * 16 >= (1L << 31)) return false;
    const int ntiles = N * (h2 / W4S_TR) * (w2 / 32);
    const long out_tiles = 2L * (Cx / 64) * jp_cdiv(Cout, 128), per = (long)Cout * 16 * Cx;
    const long sp = std::max<long>(1, std::min<long>(jp_cdiv(256, out_tiles), ntiles / 2));
    return slice_plan(p, ntiles, 8, std::min<long>(sp, ws_floats / per), 1, per);
}
template <int TR>
const char* w4s_tag() { return __PRETTY_FUNCTION__; }
// generic parity-class pass of an upsampled segment (WgradAP / WgradBP): the plan before it is forced through scratch
static inline WgradPlan parity_plan(const WgradGeom& q, long ws_floats) {
    return wgrad_plan(q.Cout, 16 * q.s[0].c, (long)q.N * (q.H / 2) * (q.W / 2), 128, 128, 3, ws_floats);
}

// ---- which kernel runs: wgrad_route alone decides, precedence is the order of its body = the order of this table.  whole = the call
// fills the whole filter bank; single = one full-resolution source tensor; without scratch (ws_floats == 0) every slice plan refuses.
// Folds: reduce4 = fold_slices, "scratch | atomic" = the plan's choice (scalar_plan / table_plan) of fold_table or the epilogue's atomics.
//   kind              predicate                                                       kernel                                    fold
//   WG_UP_HEAD        whole, up_head (one channel out of one upsampled source)        conv_small.hip                            its own
//   WG_C16            whole, one source, jp_c16_ok (16 -> 16, 3x3)                    conv_c16.hip                              its own
//   WG_SMALL_HEAD     whole, small_head (<= 4 output channels, 3x3)                   conv_small.hip                            its own
//   WG_W1             single, w1_plan (1x1 s1, Cin % 128 == 0, Cout >= 192)           jp_wgrad_w1s | w1 (JP_W9S=0)              reduce4
//   WG_W7             single, whole, w7_plan (7x7 s2 p3, 3 | 6 -> 64)                 jp_wgrad_w7<CIN>                          w7_reduce
//   WG_W9S2           single, whole, w9s2_plan (3x3 s2 p1 zero, Cout 128 | k * 256)   jp_wgrad_w9s2<KG>                         reduce4
//   WG_W9             single, w9_plan on the 64-aligned channels, X < 2 GiB,          jp_wgrad_w9s<TR, REFLECT, KG, NCB> | w9   reduce4
//                     tail 0 or (<= 32 behind >= 128)                                 (JP_W9S=0); tail: table pass              (+ table)
//   WG_CHANNEL_MAJOR  not single, Cin < 32                                            igemm WgradA x WgradB                     atomic
//   WG_SUBRANGE_TABLE not whole, Cin < 16 (the disparity channel of an iconv bank)    igemm WgradA x WgradBT1                   scratch | atomic
//   WG_UNIFORM_TAP    single, uniform_tap_ok (Cout > 64, Cin = k * 128 + (<= 32))     igemm WgradAS x WgradBUS (Cout % 8 == 0)  scratch | atomic
//                                                                                     | WgradA x WgradBU; tail: table pass      (+ table)
//   WG_BMS            single, Cin 64, or 16 | 32 with Cout <= 64; Cout % 8 == 0       igemm WgradAS x WgradBMS                  scratch | atomic
//   WG_TABLE          single                                                          igemm WgradA x WgradBT1                   scratch | atomic
//   WG_TABLE_MULTI    the rest (several sources, >= 32 channels)                      igemm WgradA x WgradBT                    atomic
// and for the upsampled segment of a per-segment call (wgrad_segments_ok; its full-resolution segments go through the table above):
//   WG_W4S            w4s_plan (Cx % 64 == 0, even half-resolution height)            jp_wgrad_w4s<TR>                          parity
//   WG_PARITY         the rest                                                        igemm WgradAP x WgradBP                   parity
enum WgradKind { WG_UP_HEAD, WG_C16, WG_SMALL_HEAD, WG_W1, WG_W7, WG_W9S2, WG_W9, WG_CHANNEL_MAJOR, WG_SUBRANGE_TABLE, WG_UNIFORM_TAP,
                 WG_BMS, WG_TABLE, WG_TABLE_MULTI, WG_W4S, WG_PARITY };
struct WgradRoute {
    WgradKind kind;
    union {             // the kind's own plan
        W1Plan w1;
        W7Plan w7;
        W9S2Plan w9s2;
        W9Plan w9;
        W4SPlan w4s;
    };
    WgradPlan gen, tab;     // generic engine: the main pass; the table pass over the channels [Cm, Cm + tail), where tail != 0
    int Cm, tail;           // channels of the main pass and of the table pass behind it (a table kind: Cm = 0, tail = all)
    bool scalar;            // the scalar-base loaders apply (WG_UNIFORM_TAP: or else the per-element ones; WG_BMS: always)
    long ws_use;            // scratch floats the route writes (the direct kernels: what their unit's query asks for)
};
// the direct kernels of conv_small.hip / conv_c16.hip
static bool wgrad_direct_route(const WgradGeom& g, WgradRoute* r) {
    const WgradGeom::Src& s = g.s[0];
    auto is = [&](WgradKind k, long use) { r->kind = k; r->ws_use = use; return true; };
    if (!g.whole()) return false;
    if (up_head(s.c, s.up, g.s[1].c, g.s[2].c, g.Cout, g.KH, g.stride, g.pad, g.pad_mode, g.H, g.W))
        return is(WG_UP_HEAD, jp_up_head_wgrad_ws_floats(g.N, s.c, g.H / 2, g.W / 2));
    if (g.one() && jp_c16_ok(s.c, g.Cout, g.KH, g.stride, g.pad, g.pad_mode, g.H, g.W))
        return is(WG_C16, jp_c16_wgrad_ws_floats(g.N, s.c, g.Cout, g.H, g.W));
    if (small_head(g.Cin(), g.Cout, g.KH, g.stride, g.pad))
        return is(WG_SMALL_HEAD, jp_conv_small_wgrad_ws_floats(g.N, g.Cin(), g.H, g.W, g.Cout, g.one() && !s.up));
    return false;
}
static WgradRoute wgrad_route(const WgradGeom& g, long ws_floats) {
    const int Cin = g.Cin(), Cout = g.Cout, KK = g.KK(), Cm = wgrad_aligned(Cin), tail = Cin - Cm;
    const bool whole = g.whole(), single = g.single();
    WgradRoute r{};
    // kind k: a main pass over cm channels that writes `use` floats of scratch, then a table pass over cn more (the scratch is free
    // again by then: the main pass has been folded on this stream)
    auto is = [&](WgradKind k, int cm, long use, int cn) {
        r.kind = k;
        r.Cm = cm;
        r.tail = cn;
        if (cn) r.tab = table_plan(g, cn, ws_floats);
        r.ws_use = std::max(use, cn && r.tab.use_ws ? r.tab.ws_need : 0);
        return r;
    };
    auto gen = [&](const WgradPlan& p) { r.gen = p; return p.use_ws ? p.ws_need : 0; };      // main pass on the generic engine
    const bool scalar_ok = Cout % 8 == 0 && (long)8 * g.H * g.W * 4 < (1L << 31);
    r.scalar = scalar_ok;
    if (wgrad_direct_route(g, &r)) return r;
    if (single && w1_plan(g, ws_floats, &r.w1)) return is(WG_W1, Cin, r.w1.need, 0);
    if (single && whole && w7_plan(g, ws_floats, &r.w7)) return is(WG_W7, Cin, r.w7.need, 0);
    if (single && whole && w9s2_plan(g, ws_floats, &r.w9s2)) return is(WG_W9S2, Cin, r.w9s2.need, 0);
    if (single && (tail == 0 || (tail <= 32 && Cm >= 128)) && (long)g.N * Cin * g.H * g.W * 4 < (1L << 31) &&
        w9_plan(g, Cm, ws_floats, &r.w9))
        return is(WG_W9, Cm, r.w9.need, tail);
    if (!single && Cin < 32) return is(WG_CHANNEL_MAJOR, Cin, gen(atomic_plan(g, KK * Cin)), 0);
    if (!whole && Cin < 16) return is(WG_SUBRANGE_TABLE, 0, 0, Cin);
    if (single && uniform_tap_ok(Cin, Cout))
        return is(WG_UNIFORM_TAP, Cm, gen(scalar_ok ? scalar_plan(g, KK * Cm, ws_floats) : atomic_plan(g, KK * Cm)), tail);
    if (single && (Cin == 64 || ((Cin == 16 || Cin == 32) && Cout <= 64)) && scalar_ok)
        return is(WG_BMS, Cin, gen(scalar_plan(g, KK * Cin, ws_floats)), 0);
    if (single) return is(WG_TABLE, 0, 0, Cin);
    return is(WG_TABLE_MULTI, Cin, gen(atomic_plan(g, KK * pad32(Cin))), 0);
}
// the upsampled segment q of a per-segment call.  WG_PARITY always reduces through scratch: where the plan would rather not, it
// takes the largest split that fits (one split needs Cout * 16 * Cx floats; the launch refuses a scratch smaller than ws_use).
static WgradRoute wgrad_up_route(const WgradGeom& q, long ws_floats) {
    WgradRoute r{};
    r.Cm = q.s[0].c;
    if (w4s_plan(q, ws_floats, &r.w4s)) {
        r.kind = WG_W4S;
        r.ws_use = r.w4s.need;
        return r;
    }
    r.kind = WG_PARITY;
    r.gen = parity_plan(q, ws_floats);
    if (!r.gen.use_ws) {
        const long Ncl = (long)q.N * (q.H / 2) * (q.W / 2), one = (long)q.Cout * 16 * q.s[0].c, chunks = jp_cdiv(Ncl, KC);
        const long sp = std::min<long>(std::max<long>(1, std::min<long>(ws_floats / one, chunks / 4)), 64);
        r.gen.kps = (int)(jp_cdiv(chunks, sp) * KC);
        r.gen.splits = jp_cdiv(Ncl, r.gen.kps);
        r.gen.ws_need = r.gen.splits * one;
    }
    r.ws_use = r.gen.ws_need;
    return r;
}

// ---- folds of the partial sums in scratch into dw
// ws[slice][co][tap * Cp + ci] of the slice kernels (W1, W9, W9S2): 8 slice lanes per output quad for few outputs and many slices
static void fold_slices(const WgradGeom& g, const float* ws, int slices, int Cp, int KHW, hipStream_t st) {
    const int nblk = (int)(((long)g.Cout * KHW * Cp / 4 + 63) / 64);
    const bool lanes8 = slices >= 64 && nblk < 2048;
    hipLaunchKernelGGL(lanes8 ? wgrad_reduce4_kernel<8> : wgrad_reduce4_kernel<1>, dim3(nblk), dim3(lanes8 ? 512 : 64), 0, st, ws, g.dw,
                       g.Cout, KHW * Cp, slices, Cp, KHW, g.dw_coff, g.dw_ctot);
}
// ws[split][co][n] of the generic engine's WgradEpiWS into the columns e describes.  wide_ok: many splits of few outputs may take
// wgrad_reduce_wide_kernel.  The scalar-base passes allow it, the table passes never did: deliberate-as-found, kept because the two
// kernels sum in different orders and so give different bits.
static void fold_table(const float* ws, const WgradEpiT& e, int M, int Np, int splits, bool wide_ok, hipStream_t st) {
    const long total = (long)M * Np;
    const bool wide = wide_ok && splits >= 32 && total <= (1L << 16);
    const dim3 grid(wide ? (int)((total + 63) / 64) : (int)std::min<long>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(wide ? wgrad_reduce_wide_kernel : wgrad_reduce_kernel, grid, dim3(wide ? 1024 : 256), 0, st, ws, e.dw, M, Np, splits,
                       e.Cp, e.Cin, e.KHW, e.c_off, e.Ctot);
}
// ws[split][co][16 * Cx] of the parity-class kernels of the upsampled segment q
static void fold_parity(const WgradGeom& q, const float* ws, int splits, hipStream_t st) {
    const long total = (long)q.Cout * q.s[0].c * 9;
    hipLaunchKernelGGL(wgrad_fold_parity_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, ws, q.dw, q.Cout,
                       q.s[0].c, splits, q.dw_coff, q.dw_ctot);
}

// ---- one launch site per route
static inline unsigned div_magic(int Cp) { return (unsigned)((1ULL << 32) / (unsigned)Cp) + 1u; }
static inline WgradA wgrad_a(const WgradGeom& g) { return WgradA{g.dy, g.Cout, (int)g.npix, g.OH * g.OW}; }
static inline WgradAS wgrad_as(const WgradGeom& g) { return WgradAS{g.dy, g.Cout, (int)g.kext(), g.OH * g.OW, g.Ppad()}; }
template <int V>
using Int = std::integral_constant<int, V>;
template <class F>
static int with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// table pass over the channels [r.Cm, r.Cm + r.tail) of a single full-resolution source (the slot tables need no channel padding)
static int run_table(const WgradGeom& g, const WgradRoute& r, float* ws, const JpCall& st) {
    const int cb = r.Cm, cn = r.tail, Np = g.KK() * cn, npix = (int)g.npix;
    const WgradPlan& p = r.tab;
    WgradEpiT e{g.dw, cn, cn, g.KK(), g.dw_coff + cb, g.dw_ctot, div_magic(cn)};
    JP_KH_SWITCH(g.KH, {
        WgradBT1<KH_> b{g.s[0].p + (size_t)cb * g.H * g.W, Np, cn, cn, g.Cin(), g.H, g.W, npix, g.OH, g.OW, g.stride, g.pad, g.reflect(),
                        div_magic(cn)};
        if (p.use_ws) launch_auto<true>(wgrad_a(g), b, WgradEpiWS{ws, g.Cout, Np}, g.Cout, Np, npix, p.splits, p.kps, st);
        else launch_auto<true>(wgrad_a(g), b, e, g.Cout, Np, npix, p.splits, p.kps, st);
    });
    if (p.use_ws) fold_table(ws, e, g.Cout, Np, p.splits, false, st);
    return JP_OK;
}
// scalar-base main pass under r.gen (scalar_plan)
template <int WM, int WN, class B>
static void run_scalar(B b, const WgradEpiT& e, int Np, const WgradGeom& g, const WgradPlan& p, float* ws, const JpCall& st) {
    if (!p.use_ws) return launch<true, WM, WN>(wgrad_as(g), b, e, g.Cout, Np, (int)g.kext(), p.splits, p.kps, st);
    launch<true, WM, WN>(wgrad_as(g), b, WgradEpiWS{ws, g.Cout, Np}, g.Cout, Np, (int)g.kext(), p.splits, p.kps, st);
    fold_table(ws, e, g.Cout, Np, p.splits, true, st);
}
static void run_w1(const WgradGeom& g, const W1Plan& p, float* ws, const JpCall& st) {
    const int N = g.N, Cin = g.Cin(), H = g.H, W = g.W, Cout = g.Cout, dyb = (int)((long)N * Cout * H * W * 4);
    const dim3 grid(Cin / 128, jp_cdiv(Cout, 256), p.splits);
    if (w9s_enabled()) {    // W1S: the same tile and split-K plan on the bf16 pipe (igemm_w9s.h)
        const WgradAmax am = wgrad_amax(g, st);
        jp_prof_before(w1s_tag(), JP_NPROD * 2.0 * Cout * (double)Cin * N * H * W, st);
        hipLaunchKernelGGL(jp_wgrad_w1s_kernel, grid, dim3(512), 0, st, g.dy, g.s[0].p, ws, Cout, Cin, Cin, H, W, p.ntiles, p.tps, dyb,
                           am.g, am.x);
    } else {
        jp_prof_before(w1_tag(), 2.0 * Cout * (double)Cin * N * H * W, st);
        hipLaunchKernelGGL(jp_wgrad_w1_kernel, grid, dim3(512), 0, st, g.dy, g.s[0].p, ws, Cout, Cin, Cin, H, W, p.ntiles, p.tps, dyb);
    }
    jp_prof_after(st);
    fold_slices(g, ws, p.splits, Cin, 1, st);
}
// channel-major (WG_CHANNEL_MAJOR: few channels) or slot-table (WG_TABLE_MULTI: channels padded to 32) gather from any source layout
static int run_multi(const WgradGeom& g, const WgradRoute& r, const JpCall& st) {
    const int Cin = g.Cin(), Cp = pad32(Cin), Kw = Cin * g.KK(), Np = g.KK() * Cp, npix = (int)g.npix;
    const WgradGeom::Src* s = g.s;
    const Src3 src = make_src(s[0].p, s[0].c, s[0].up, s[1].p, s[1].c, s[1].up, s[2].p, s[2].c, s[2].up, g.H, g.W);
    JP_KH_SWITCH(g.KH, {
        if (r.kind == WG_CHANNEL_MAJOR) {
            WgradB<KH_> b{src, Kw, npix, g.OH, g.OW, g.stride, g.pad, g.reflect()};
            launch_auto<true>(wgrad_a(g), b, WgradEpi{g.dw, Kw}, g.Cout, Kw, npix, r.gen.splits, r.gen.kps, st);
        } else {
            WgradBT<KH_> b{src, Np, Cp, Cin, npix, g.OH, g.OW, g.stride, g.pad, g.reflect(), div_magic(Cp)};
            WgradEpiT e{g.dw, Cp, Cin, g.KK(), 0, Cin, div_magic(Cp)};
            launch_auto<true>(wgrad_a(g), b, e, g.Cout, Np, npix, r.gen.splits, r.gen.kps, st);
        }
    });
    return JP_OK;
}
// BMS, 16 / 32 / 64 input channels (ResNet stem + layer1, BEV decoder): f(WM, WN, TPT, CPT), the GEMM tile and the whole taps per N tile
template <class F>
static int bms_shape(int Cin, bool narrow, F&& f) {
    if (Cin == 16) return f(Int<1>{}, Int<4>{}, Int<16>{}, Int<16>{});
    if (Cin == 32) return f(Int<1>{}, Int<4>{}, Int<8>{}, Int<32>{});
    return narrow ? f(Int<1>{}, Int<4>{}, Int<4>{}, Int<64>{}) : f(Int<2>{}, Int<2>{}, Int<2>{}, Int<64>{});
}
// main pass over the r.Cm aligned channels (WG_BMS: all of them; WG_UNIFORM_TAP: one filter tap per 128-wide N tile, scalar-base or
// per-element loaders), then a table pass for the tail
static int run_aligned(const WgradGeom& g, const WgradRoute& r, float* ws, const JpCall& st) {
    const int Cm = r.Cm, Np = g.KK() * Cm, Cin = g.Cin(), npix = (int)g.npix;
    const float* x = g.s[0].p;
    WgradEpiT e{g.dw, Cm, Cm, g.KK(), g.dw_coff, g.dw_ctot, div_magic(Cm)};
    const int rc = with_bool(g.reflect(), [&](auto refl) {
        if (r.kind == WG_BMS)
            return bms_shape(Cin, scalar_narrow(g), [&](auto wm, auto wn, auto tpt, auto cpt) {
                JP_KH_SWITCH(g.KH, {
                    WgradBMS<KH_, refl(), tpt(), cpt()> b{x, Cin, g.H, g.W, g.OH, g.OW, g.stride, g.pad, g.Ppad()};
                    run_scalar<wm(), wn()>(b, e, Np, g, r.gen, ws, st);
                });
                return JP_OK;
            });
        JP_KH_SWITCH(g.KH, {
            if (r.scalar) {
                WgradBUS<KH_, refl()> b{x, Cm, Cin, g.H, g.W, g.OH, g.OW, g.stride, g.pad, g.Ppad()};
                run_scalar<2, 2>(b, e, Np, g, r.gen, ws, st);
            } else {
                WgradBU<KH_> b{x, Cm, Cm, Cin, g.H, g.W, npix, g.OH, g.OW, g.stride, g.pad, g.reflect()};
                launch<true, 2, 2>(wgrad_a(g), b, e, g.Cout, Np, npix, r.gen.splits, r.gen.kps, st);
            }
        });
        return JP_OK;
    });
    if (rc || !r.tail) return rc;
    return run_table(g, r, ws, st);
}

// wgrad of g's sources into their dw columns.  Sub-range calls (dw_coff > 0 or fewer channels than dw_ctot) must be single-source.
static int wgrad_impl(const WgradGeom& g, float* ws, long ws_floats, const JpCall& st) {
    JP_CHECK_ARG(g.npix < (1L << 31), "conv2d_wgrad: tensor too large");
    JP_CHECK_ARG(g.whole() || g.single(), "conv2d_wgrad: internal sub-range call must be single-source");
    if (!ws) ws_floats = 0;
    const WgradRoute r = wgrad_route(g, ws_floats);
    // (the direct kernels size themselves: their ws_use is their unit's wish, and they run with less)
    JP_CHECK_ARG(r.kind <= WG_SMALL_HEAD || r.ws_use <= std::max(ws_floats, 0L),
                 "conv2d_wgrad: internal: the route plans more scratch than it was given");
    const WgradGeom::Src* s = g.s;
    int rc = JP_OK;
    switch (r.kind) {
        case WG_UP_HEAD: rc = jp_up_head_wgrad(s[0].p, g.dy, g.dw, g.N, s[0].c, g.H / 2, g.W / 2, st, ws, ws_floats); break;
        case WG_C16: rc = jp_c16_wgrad(s[0].p, s[0].up, g.dy, g.dw, g.N, s[0].c, g.Cout, g.H, g.W, st, ws, ws_floats); break;
        case WG_SMALL_HEAD:
            rc = jp_conv_small_wgrad(s[0].p, s[0].c, s[0].up, s[1].p, s[1].c, s[1].up, s[2].p, s[2].c, s[2].up, g.dy, g.dw, g.N, g.H,
                                     g.W, g.Cout, g.reflect(), st, ws, ws_floats);
            break;
        case WG_W1: run_w1(g, r.w1, ws, st); break;
        case WG_W7: (s[0].c == 3 ? launch_w7<3> : launch_w7<6>)(g, r.w7, ws, st); break;
        case WG_W9S2:
            (r.w9s2.kg == 2 ? launch_w9s2<2> : launch_w9s2<1>)(g, r.w9s2, ws, st);
            fold_slices(g, ws, r.w9s2.slices, s[0].c, 9, st);
            break;
        case WG_W9:     // input patch staged once per pixel tile for all 9 taps, dY fragments straight from global memory
            (g.reflect() ? launch_w9<true> : launch_w9<false>)(g, r.Cm, r.w9, ws, st);
            fold_slices(g, ws, r.w9.slices, r.Cm, 9, st);
            if (r.tail) rc = run_table(g, r, ws, st);
            break;
        case WG_CHANNEL_MAJOR:
        case WG_TABLE_MULTI: rc = run_multi(g, r, st); break;
        case WG_UNIFORM_TAP:
        case WG_BMS: rc = run_aligned(g, r, ws, st); break;
        case WG_SUBRANGE_TABLE:
        case WG_TABLE: rc = run_table(g, r, ws, st); break;
        default:      // (WG_W4S, WG_PARITY: wgrad_up_route's kinds, run_up_segment)
            jp_set_last_error("conv2d_wgrad: internal: not a kind of wgrad_route");
            rc = JP_EBADARG;
            break;
    }
    if (rc) return rc;
    JP_LAUNCH_CHECK();
}
// the upsampled segment q of a per-segment call: 16 (class, slot) GEMMs over the half-resolution pixels
static int run_up_segment(const WgradGeom& q, float* ws, long ws_floats, const JpCall& st) {
    const WgradRoute r = wgrad_up_route(q, ws_floats);
    JP_CHECK_ARG(r.ws_use <= ws_floats, "conv2d_wgrad: scratch too small (jp_conv2d_wgrad_src3_ws_floats)");
    const int N = q.N, H = q.H, W = q.W, Cout = q.Cout, h2 = H / 2, w2 = W / 2, Cx = q.s[0].c, Np = 16 * Cx;
    const long Ncl = (long)N * h2 * w2;
    if (r.kind == WG_W4S) {
        const WgradAmax am = wgrad_amax(q, st);
        jp_prof_before(w4s_tag<W4S_TR>(), JP_NPROD * 2.0 * Cout * 16.0 * Cx * (double)Ncl, st);
        hipLaunchKernelGGL((jp_wgrad_w4s_kernel<W4S_TR>), dim3(Cx / 64, jp_cdiv(Cout, 128), 2 * r.w4s.splits), dim3(512), 0, st, q.dy,
                           q.s[0].p, ws, Cout, Cx, h2, w2, r.w4s.ntiles, r.w4s.tps, (int)((long)N * Cout * H * W * 4), am.g, am.x);
        jp_prof_after(st);
    } else {
        launch<true, 2, 2>(WgradAP{q.dy, Cout, h2, w2, 4 * Cx}, WgradBP{q.s[0].p, Cx, h2, w2}, WgradEpiWS{ws, Cout, Np}, Cout, Np,
                           (int)Ncl, r.gen.splits, r.gen.kps, st);
    }
    fold_parity(q, ws, r.kind == WG_W4S ? r.w4s.splits : r.gen.splits, st);
    return JP_OK;
}
// the sources are eligible for the per-segment wgrad (no materialised concat): full-resolution segments run the
// single-source routes on their own tensor, the upsampled one the parity-class kernels
static bool wgrad_segments_ok(const WgradGeom& g) {
    int nseg = 0, nup = 0, cup = 0;     // segments, upsampled ones, channels of the (one) upsampled segment
    for (const WgradGeom::Src& s : g.s) {
        nseg += s.c != 0;
        if (s.c && s.up) {
            ++nup;
            cup = s.c;
        }
    }
    return nseg >= 2 && nup == 1 && cup % 128 == 0 && g.Cout % 8 == 0 && g.Cout > 64 && g.KH == 3 && g.stride == 1 && g.pad == 1 &&
           g.reflect() && g.H % 2 == 0 && (g.W / 2) % 32 == 0 && g.W % 2 == 0 && (long)g.N * g.H * g.W < (1L << 31);
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
    const WgradGeom g = wgrad_geom({x0, c0, up0}, {x1, c1, up1}, {x2, c2, up2}, dy, dw, N, H, W, Cout, KH, stride, pad, pad_mode);
    if (!accumulate) JP_HIP(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)Cout * g.Cin() * KH * KH, st));
    if (!(ws && wgrad_segments_ok(g))) return wgrad_impl(g, ws, ws_floats, st);
    for (int i = 0, coff = 0; i < 3; coff += g.s[i++].c) {
        if (!g.s[i].c) continue;
        const WgradGeom q = wgrad_segment(g, i, coff);
        const int rc = q.s[0].up ? run_up_segment(q, ws, ws_floats, st) : wgrad_impl(q, ws, ws_floats, st);
        if (rc) return rc;
    }
    JP_LAUNCH_CHECK();
}

// scratch floats for jp_conv2d_wgrad_src3 on a multi-source input (0 = use the single-source query / no benefit).  Per-segment calls:
// a maximum over the kernels the segments may run under a 48 Mi cap (each route adapts its split count to the scratch it is given).
extern "C" long jp_conv2d_wgrad_src3_ws_floats(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W,
                                               int Cout, int KH, int stride, int pad, int pad_mode) {
    const WgradGeom g = wgrad_geom({nullptr, c0, up0}, {nullptr, c1, up1}, {nullptr, c2, up2}, nullptr, nullptr, N, H, W, Cout, KH,
                                   stride, pad, pad_mode);
    WgradRoute r{};
    if (wgrad_direct_route(g, &r)) return r.ws_use;
    if (!wgrad_segments_ok(g)) return 0;
    const long cap = 48L << 20;
    long need = 0;
    for (int i = 0; i < 3; ++i) {
        const WgradGeom q = wgrad_segment(g, i, 0);
        const int c = q.s[0].c;
        if (c && q.s[0].up) {
            const WgradPlan p = parity_plan(q, cap);
            need = std::max(need, p.use_ws ? p.ws_need : (long)Cout * 16 * c);
            if (w4s_plan(q, cap, &r.w4s)) need = std::max(need, r.w4s.need);
        } else if (c >= 16) {
            const WgradPlan p = scalar_plan(q, g.KK() * wgrad_aligned(c), cap);
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
// reduction pass instead of device-scope atomics (0 = no benefit for this shape).  Capped at 32 Mi floats.  Past the direct kernels
// and W7 the answer is a maximum over the candidate routes, not the need of the route taken: the query knows neither pad_mode nor
// whether the call will be given scratch at all, and each route adapts its split count to what it gets.  The slot-table candidate
// (fixed-order fold of odd channel counts, Cout % 8 != 0, the 1-channel tail of the 513-channel banks) is the uniform-tap tail or all.
extern "C" long jp_conv2d_wgrad_ws_floats(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad) {
    const WgradGeom g = wgrad_geom({nullptr, Cin, 0}, {nullptr, 0, 0}, {nullptr, 0, 0}, nullptr, nullptr, N, H, W, Cout, KH, stride,
                                   pad, JP_PAD_ZERO);
    const long cap = 32L << 20;
    WgradRoute r{};
    if (wgrad_direct_route(g, &r)) return r.ws_use;
    if (w7_plan(g, cap, &r.w7)) return r.w7.need;
    const long need1 = w1_plan(g, cap, &r.w1) ? r.w1.need : 0;
    const int tail = uniform_tap_ok(Cin, Cout) ? Cin % 128 : 0;
    const WgradPlan pt = table_plan(g, tail ? tail : Cin, cap), p = scalar_plan(g, g.KK() * wgrad_aligned(Cin), cap);
    const long need_t = pt.use_ws ? pt.ws_need : 0;
    if (Cout % 8 != 0 || Cin < 16) return need_t;
    const long need9 = w9_plan(g, wgrad_aligned(Cin), cap, &r.w9) ? r.w9.need : 0;
    const long need92 = w9s2_plan(g, cap, &r.w9s2) ? r.w9s2.need : 0;
    return std::max({p.use_ws ? p.ws_need : 0L, need9, need1, need92, need_t});
}
