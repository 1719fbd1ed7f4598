// conv2d dgrad: jp_conv2d_dgrad, jp_conv2d_dgrad_src3, their scratch-size queries, the reflection border and upsample edge passes,
// and the loaders and epilogues that only dgrad instantiates (conv_fwd.hip's head has the GEMM shapes and the loader families).
// The patch-kernel launch layer it shares with the forward is in conv_launch.h.
#include "conv_launch.h"
#include "igemm_p9sd.h"
#include "igemm_p9s2d.h"

namespace {

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

// P9SD (igemm_p9sd.h): dgrad of the upsampled iconv segment at half resolution on the bf16 pipe; JP_P9SD=0 keeps DgradUPB
inline bool p9sd_enabled() {
    static const int on = [] { const char* e = getenv("JP_P9SD"); return e ? atoi(e) : 1; }();
    return on != 0;
}
template <class E>
const char* p9sd_tag() { return __PRETTY_FUNCTION__; }
template <int WM, int WN, class E>
const char* p9s2d_tag() { return __PRETTY_FUNCTION__; }

}  // namespace

// ---- geometry of one input-gradient call, read by every route predicate, plan and launcher (the scratch queries: no pad mode, every
// scratch given).  For a per-source call it describes the whole bank (Cin = all sources' channels).
struct KSlices {
    int kps, n;     // K per slice (a multiple of KC) and the slices that gives
};
static inline KSlices k_slices(int Kp, int sp) {
    const int kps = jp_cdiv(jp_cdiv(Kp, sp), KC) * KC;
    return KSlices{kps, jp_cdiv(Kp, kps)};
}
struct DgradGeom {
    int N, Cin, H, W, Cout, KH, stride, pad, pad_mode;
    bool has_ws, has_split;     // the pack scratch `ws` / the split scratch `split_ws` were given
    int OH, OW, Cp, Kp;
    long npix;
    int KK() const { return KH * KH; }
    bool reflect() const { return pad_mode == JP_PAD_REFLECT; }
    bool s1_3x3() const { return KH == 3 && stride == 1 && pad == 1; }
    bool halves() const { return H % 2 == 0 && W % 2 == 0 && 2 * OH == H && 2 * OW == W; }      // an even map onto exactly its half
    // 3x3 stride 2 pad 1 on an even map; s2_parity: and the pixels of one parity class fill whole 256-pixel tiles (the generic
    // parity-class form; maps it does not take, e.g. the 8 x 8 maps of the 256^2 test shapes, run the plain loader)
    bool s2_form() const { return KH == 3 && stride == 2 && pad == 1 && !reflect() && halves(); }
    long Nc() const { return (long)N * (H / 2) * (W / 2); }
    bool s2_parity() const { return s2_form() && Nc() % 256 == 0; }
    // rows of a short row tail, 0 = none: 513 = 4*128 + 1 input channels of the iconv layers run the tail as its own 64-row launch
    // instead of a fifth, almost empty 128-row tile column
    int tail() const { return (Cin > 128 && Cin % 128 <= 16) ? Cin % 128 : 0; }
    int small_grid() const { return small_grid_splits(Cin, npix, Kp); }      // K slices of a tile grid that cannot fill the chip
    int ring(int h, int w) const { return N * (2 * w + 2 * h); }             // border-adjacent (edge) pixels of the N (h, w) maps
};
static DgradGeom dgrad_geom(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad, int pad_mode, bool has_ws,
                            bool has_split) {
    DgradGeom g{N, Cin, H, W, Cout, KH, stride, pad, pad_mode, has_ws, has_split};
    g.OH = stride > 0 ? (H + 2 * pad - KH) / stride + 1 : 0;
    g.OW = stride > 0 ? (W + 2 * pad - KH) / stride + 1 : 0;
    g.Cp = pad32(Cout);
    g.Kp = KH * KH * g.Cp;
    g.npix = (long)N * H * W;
    return g;
}
// the row-tile kernel takes M rows of a 3x3 stride-1 bank: whole 256- (up to 64 rows) or 128-pixel tiles per image row
static inline bool row_tile_ok(const DgradGeom& g, int M) {
    return g.s1_3x3() && g.Cout >= 32 && g.W % (M <= 64 ? 256 : 128) == 0 && g.npix > 64;
}

// ---- split plan of the ring passes: the reflection border pass of a full-resolution bank (C rows over the Nb border-adjacent pixels)
// and the edge pass of an upsampled segment (over the Nb boundary pixels of the half-resolution map).  Their cost is the scattered
// read-modify-write of the epilogue, not the K loop (border_splits), so K is split only for a few dozen tiles.  Given scratch, the
// slices are stored (coalesced along the ring) and ONE small pass folds them into dx in a fixed order; without it they meet in the
// epilogue's atomics.  The two passes wish for slices differently, as found: the border pass asks for up to `cap` slices of at least
// 9 chunks while that gives fewer than `floor` tiles, whatever the epilogue would do; the edge pass (16 slots x Cout: a long K loop
// of branchy gathers) splits for the epilogue up to 4 ways below `floor` tiles and sends at most `cap` of those slices to scratch.
struct RingPolicy {
    int cap, floor;
    bool from_epilogue;
};
constexpr RingPolicy BORDER_RING{4, 512, false}, EDGE_RING{8, 256, true};
struct RingPlan {
    KSlices sl;
    bool scratch;       // through split_ws and the fold kernel; else the read-modify-write epilogue (atomic where sl.n > 1)
};
static RingPlan ring_plan(int C, int Nb, int Kp, bool scratch_given, const RingPolicy& pol) {
    const long btiles = (long)jp_cdiv(C, C <= 64 ? 64 : 128) * jp_cdiv(Nb, C <= 64 ? 256 : 128);
    const int chunks = Kp / KC;
    int esp = border_splits(btiles, chunks), wish;
    if (pol.from_epilogue) {
        esp = (int)std::max<long>(esp, std::min<long>(4, jp_cdiv(pol.floor, btiles)));
        wish = std::min(k_slices(Kp, esp).n, pol.cap);
    } else {
        wish = (int)std::max<long>(1, std::min<long>(std::min<long>(pol.cap, chunks / 9), jp_cdiv(pol.floor, btiles)));
    }
    const bool scratch = scratch_given && wish > 1;
    return RingPlan{k_slices(Kp, scratch ? wish : esp), scratch};
}
static inline long ring_floats(const RingPlan& p, int C, int Nb) { return p.scratch ? (long)p.sl.n * C * Nb : 0; }
static inline bool border_via_ws() {
    static const bool on = [] { const char* e_ = getenv("JP_BORDER_WS"); return !(e_ && e_[0] == '0'); }();
    return on;
}
static inline RingPlan border_plan(const DgradGeom& g, int C) {
    return ring_plan(C, g.ring(g.H, g.W), g.Kp, border_via_ws() && g.has_split, BORDER_RING);
}
static inline RingPlan edge_plan(const DgradGeom& g, int C) { return ring_plan(C, g.ring(g.H / 2, g.W / 2), 16 * g.Cp, g.has_split, EDGE_RING); }

// ---- which kernel runs: dgrad_route alone decides for jp_conv2d_dgrad, precedence is the order of its body = the order of this table.
// Every kind between DG_C16 and DG_CHANNEL_MAJOR needs the pack scratch `ws` and Cout >= 16.  s2 form = 3x3 stride 2 pad 1 on an even
// map; sp = small_grid_splits of the tile grid; tail = the 1 channel of 513 (DgradGeom::tail), run by a launch of its own on the same
// pack (DgradBT x DgradEpi) behind the main pass over the other Mm rows.  A reflection layer (3x3 stride 1) is followed by the border
// pass (ring_plan: through scratch and border_add_kernel, or its read-modify-write epilogue) behind every kind from DG_P9SM down to
// DG_TAP.  Packs: T = tap-major (pack_weights), F = fragment-order behind it (pack_p9), built when ws_state == 0.
//   kind              predicate                                                          kernel                                 packs  fold
//   DG_C16            jp_c16_ok (16 -> 16, 3x3)                                          conv_c16.hip                           -      -
//   DG_P9S2D          s2 form, JP_P9S / JP_P9S2 / JP_P9S2D on, Cin >= 32, Cout % 16 == 0, jp_igemm_p9s2d_kernel<1, 4 | 2, 2>     F      -
//                     OW % 32 == 0, OH % (8 | 4) == 0, dY < 2 GiB, >= 192 workgroups
//   DG_P1S2           1x1 stride 2 pad 0 on an even map, p1s2_ok                         launch_p9s<DgradS2PointEpi, 1>         F      -
//   DG_S2_PARITY      s2 form, N * H/2 * W/2 % 256 == 0                                  igemm PackAS2 x DgradS2B               T      -
//   DG_P9SM           no tail, p9sm_wanted, one split or split_ws given                  jp_p9sm_launch                         T F    slice_reduce_nchw
//   DG_SPLIT_SCRATCH  sp > 1, split_ws given                                             igemm PackA x DgradBT -> WgradEpiWS    T      slice_reduce_nchw
//   DG_SPLIT_ATOMIC   sp > 1                                                             memset, the same -> AtomicEpi          T      atomics
//   DG_P1             stride 1, 1x1 pad 0, no tail, p9_ok(Cin, .., 1)                    launch_p1                              T F    -
//   DG_P9 (+ tail)    3x3 stride 1 pad 1, tail 0 or Mm > 64, p9_ok(Mm, ..)               launch_p9<false, true>                 (T) F  -
//                                                                                        (T: only for a tail or a border pass)
//   DG_ROW_TILE (+ tail)  row_tile_ok(Mm): 3x3 stride 1 pad 1, Cout >= 32,                   launch_r3<1, 4 | 2, 2>                 T      -
//                     W % (256 | 128) == 0, > 64 pixels
//   DG_TAP (+ tail)   the rest, either stride                                            igemm PackA x DgradBT<KH, S1>          T      -
//   DG_CHANNEL_MAJOR  no ws, or Cout < 16                                                igemm DgradA x DgradB                  -      -
// and for the sources of a per-source call (dgrad_src3_route: unless the whole call is the up-head, Src3Route::up_head, one kind per
// segment; a source whose gradient is not wanted is DG_NONE).  Full-resolution segments, each followed by the border pass over its rows:
//   DG_SMALL          C <= 4 (the disparity channel)                                     conv_small.hip on flipped taps
//   DG_P9             Cin > 64, C > 64 at a multiple of the bank's M tile, p9_ok(C, ..)  launch_p9 on the bank's F pack, from tile coff / bmt
//   DG_ROW_TILE       row_tile_ok(C)                                                     launch_r3
//   DG_TAP            the rest                                                           igemm PackA x DgradBT<3, true>
// the upsampled segment, followed by the edge pass (ring_plan: through scratch and edge_add_kernel, or the atomic epilogue):
//   DG_P9SD           JP_P9SD on, h2 % 4 == 0, w2 % 32 == 0, Cout % 16 == 0, dY < 2 GiB, >= 192 workgroups  jp_igemm_p9sd_kernel
//   DG_UP_TAP         the rest                                                           igemm PackA x DgradUPB
enum DgradKind { DG_C16, DG_P9S2D, DG_P1S2, DG_S2_PARITY, DG_P9SM, DG_SPLIT_SCRATCH, DG_SPLIT_ATOMIC, DG_P1, DG_P9, DG_ROW_TILE, DG_TAP,
                 DG_CHANNEL_MAJOR, DG_NONE, DG_SMALL, DG_P9SD, DG_UP_TAP };
struct DgradRoute {
    DgradKind kind;
    int Mm, tail;           // rows of the main pass and of the tail launch behind it
    KSlices sl;             // DG_SPLIT_*: the small-grid slices
    JpP9smPlan sm;          // DG_P9SM
    bool pack_tap;          // the route reads the tap-major pack (as found, also built for DG_P9SM, which reads it in the border pass only, and DG_P1)
    int frag_bmt, frag_khw; // ... the fragment-order pack with this M tile and tap count (frag_bmt == 0: none)
    bool border;            // a reflection border pass follows, planned by `ring`
    RingPlan ring;
    long split_use;         // floats of split_ws the route writes (jp_conv2d_dgrad_split_floats answers at least this)
};
static DgradRoute dgrad_route(const DgradGeom& g) {
    const int N = g.N, Cin = g.Cin, H = g.H, W = g.W, Cout = g.Cout, OH = g.OH, OW = g.OW;
    DgradRoute r{};
    r.Mm = Cin;
    auto is = [&](DgradKind k, bool tap, int frag_bmt, int frag_khw, long use) {
        r.kind = k;
        r.pack_tap = tap;
        r.frag_bmt = frag_bmt;
        r.frag_khw = frag_khw;
        r.border = g.reflect() && k >= DG_P9SM && k <= DG_TAP;
        if (r.border) r.ring = border_plan(g, Cin);
        r.split_use = std::max(use, r.border ? ring_floats(r.ring, Cin, g.ring(H, W)) : 0);
        return r;
    };
    if (jp_c16_ok(Cin, Cout, g.KH, g.stride, g.pad, g.pad_mode, H, W)) return is(DG_C16, false, 0, 0, 0);
    if (!(g.has_ws && Cout >= 16)) return is(DG_CHANNEL_MAJOR, false, 0, 0, 0);
    // 3x3 stride-2 layers: class-uniform split-bf16 kernel on the half-resolution grid (its own fragment-order pack only)
    const int tr2 = Cin <= 64 ? 8 : 4, bm2 = Cin <= 64 ? 64 : 128;
    if (g.s2_form() && p9s_enabled() && p9s2_enabled() && JP_ENV_ON("JP_P9S2D") && Cin >= 32 && Cout % 16 == 0 && OW % 32 == 0 &&
        OH % tr2 == 0 && (long)N * Cout * OH * OW * 4 < (1L << 31) && (long)jp_cdiv(Cin, bm2) * N * (OH / tr2) * (OW / 32) * 4 >= 192)
        return is(DG_P9S2D, false, bm2, 9, 0);
    // 1x1 stride 2: the stride-1 1x1 kernel over the half-resolution dY, scattering epilogue
    if (g.KH == 1 && g.stride == 2 && g.pad == 0 && g.halves() && p1s2_ok(Cin, Cout, N, OH, OW))
        return is(DG_P1S2, false, p9_bmt(Cin, 1, p9_ptiles(N, OH, OW)), 1, 0);
    if (g.s2_parity()) return is(DG_S2_PARITY, true, 0, 0, 0);       // 4 tap slots instead of 9 taps per input pixel
    // small maps: main pass on the split-bf16 patch kernel (taps mirrored, zero fill), then the reflection fold as usual
    const int tail = g.tail();
    if (!tail && p9sm_wanted(Cin, Cout, N, H, W, g.KH, g.stride, g.pad, &r.sm) && (r.sm.splits == 1 || g.has_split))
        return is(DG_P9SM, true, r.sm.bmt, g.KK(), r.sm.part_floats);
    // small grids: K slices to scratch and a fixed-order reduction (no memset, no atomics), or into a zeroed dx by atomics
    const int sp = g.small_grid();
    if (sp > 1) {
        r.sl = k_slices(g.Kp, sp);
        return g.has_split ? is(DG_SPLIT_SCRATCH, true, 0, 0, (long)r.sl.n * Cin * g.npix) : is(DG_SPLIT_ATOMIC, true, 0, 0, 0);
    }
    // the main launch covers the first Mm rows; a row tail is finished by its own launch on the same pack
    r.tail = tail;
    r.Mm = Cin - tail;
    if (g.stride == 1) {
        if (g.KH == 1 && g.pad == 0 && tail == 0 && p9_ok(Cin, Cout, N, H, W, 1)) return is(DG_P1, true, p9_bmt(Cin, 1, p9_ptiles(N, H, W)), 1, 0);
        // P9 patch kernel on dY (taps mirrored, zero fill; the reflection fold stays with the border pass).  With a short row tail
        // (513 = 4*128 + 1) the kernel runs the full 128-row tiles of the whole bank's pack.  A zero-padded layer it covers completely
        // never reads the tap-major pack: that is neither built nor replayed for it.
        if (g.s1_3x3() && (tail == 0 || r.Mm > 64) && p9_ok(r.Mm, Cout, N, H, W))
            return is(DG_P9, tail || g.reflect(), p9_bmt(Cin, 9, p9_ptiles(N, H, W)), 9, 0);
        if (row_tile_ok(g, r.Mm)) return is(DG_ROW_TILE, true, 0, 0, 0);
    }
    return is(DG_TAP, true, 0, 0, 0);
}

// Scratch queries.  A query has no pad mode and cannot know whether the scratch will come: it answers for a call that gets it, and
// returns the maximum over the candidates its arguments leave open -- the border pass at its cap for every 3x3 stride-1 pad-1 layer,
// the small-map plan whether or not the launch side prefers another kernel, the small-grid slices.  ops.py allocates by these numbers.
// floats of jp_conv2d_dgrad's optional `split_ws` (as jp_conv2d_fwd_split_floats, conv_fwd.hip, for the forward)
extern "C" long jp_conv2d_dgrad_split_floats(int N, int Cin, int H, int W, int Cout, int KH, int stride, int pad) {
    if (Cout < 16) return 0;
    const DgradGeom g = dgrad_geom(N, Cin, H, W, Cout, KH, stride, pad, JP_PAD_ZERO, true, true);
    // the parity-class forms need no split; the stride-2 maps they do not take run the generic loader, whose small-grid K slices
    // must not meet in atomics (that was the first run-dependent sum of the backward at those shapes, tools/debug/first_divergence.py)
    if (g.s2_parity()) return 0;
    long need = g.s1_3x3() ? (long)BORDER_RING.cap * Cin * N * (2L * H + 2L * W) : 0;
    JpP9smPlan sm;
    if (p9sm_wanted(Cin, Cout, N, H, W, KH, stride, pad, &sm)) need = std::max(need, sm.part_floats);
    const int sp = g.small_grid();
    if (sp > 1) need = std::max(need, (long)k_slices(g.Kp, sp).n * Cin * g.npix);
    return need;
}

// ---- ring passes
// reflection border pass of a dgrad (rows of `a` = the C input channels of this call).  The fold reports max |final value| of the
// pixels it touches into the slot the main pass reported into (every element of dx is then covered by one of the two); the
// read-modify-write epilogue does not report: the caller reduces dx itself
static void border_pass(const PackA& a, const float* dy, float* dx, int C, const DgradGeom& g, const RingPlan& p, float* split_ws,
                        const JpCall& st) {
    const int Nb = g.ring(g.H, g.W);
    DgradBorderB<3> bb{dy, g.Cp, Nb, g.H, g.W, g.Cout};
    if (p.scratch) {      // (also the one-row launches -- the disparity channel)
        WgradEpiWS es{split_ws, C, Nb};
        launch_auto(a, bb, es, C, Nb, g.Kp, p.sl.n, p.sl.kps, st);
        const long total = (long)C * Nb;
        hipLaunchKernelGGL(border_add_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, split_ws, dx, C, Nb, g.H,
                           g.W, p.sl.n, (st.ax && st.ax->out_taken) ? st.ax->out : nullptr);
        return;
    }
    if (st.ax) st.ax->out_taken = false;
    DgradBorderEpi be{dx, C, g.H, g.W, Nb, p.sl.n > 1};
    launch_auto(a, bb, be, C, Nb, g.Kp, p.sl.n, p.sl.kps, st);
}
// edge pass of the upsampled segment (rows of `a` = its C channels, [16][C][Cp] pack): the clamp-folded entries of the boundary lines.
// Through scratch the slices never meet in float atomics (run-dependent last bits in the gradient of the upsampled segment, which the
// whole coarser decoder level inherits)
static void edge_pass(const PackA& a, const float* dy, float* dx, int C, const DgradGeom& g, const RingPlan& p, float* split_ws,
                      const JpCall& st) {
    const int h2 = g.H / 2, w2 = g.W / 2, Nb = g.ring(h2, w2), KpU = 16 * g.Cp;
    DgradUPBorderB bb{dy, Nb, h2, w2, g.Cout};
    if (p.scratch) {
        WgradEpiWS es{split_ws, C, Nb};
        launch_auto(a, bb, es, C, Nb, KpU, p.sl.n, p.sl.kps, st);
        const long total = (long)C * Nb;
        hipLaunchKernelGGL(edge_add_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, split_ws, dx, C, Nb, h2,
                           w2, p.sl.n);
        return;
    }
    DgradEdgeEpi be{dx, C, h2, w2, Nb, p.sl.n > 1};
    launch_auto(a, bb, be, C, Nb, KpU, p.sl.n, p.sl.kps, st);
}

// ---- launch sites
// main pass over M rows of a full-resolution 3x3 stride-1 bank (DG_P9, DG_ROW_TILE) or of any bank (DG_TAP): `a` = the rows' slice of
// the bank's tap-major pack, wfr = the bank's fragment-order pack, of which the rows start at M tile mt_off
template <class B>
static void main_pass(DgradKind kind, const PackA& a, const float* wfr, int mt_off, B b, DgradEpi e, int M, const DgradGeom& g,
                      const float* dy, const JpCall& st) {
    const int npix = (int)g.npix;
    if (kind == DG_P9) {
        launch_p9<false, true>(wfr, dy, e, M, g.Cout, g.N, g.H, g.W, st, mt_off, g.Cin);
    } else if (kind == DG_ROW_TILE) {      // (taps mirrored, zero fill; the reflection fold stays with the border pass)
        const Src3 sdy = make_src(dy, g.Cout, 0, nullptr, 0, 0, nullptr, 0, 0, g.H, g.W);
        if (M <= 64) { FwdBR3<false, true, 256> b3{sdy, g.H, g.W}; launch_r3<1, 4>(a, b3, e, M, npix, g.Kp, st); }
        else { FwdBR3<false, true, 128> b3{sdy, g.H, g.W}; launch_r3<2, 2>(a, b3, e, M, npix, g.Kp, st); }
    } else {
        launch_auto(a, b, e, M, npix, g.Kp, 1, g.Kp, st);
    }
}
// DG_P9 / DG_ROW_TILE / DG_TAP of jp_conv2d_dgrad: the main pass over r.Mm rows, then the row tail
static int run_rows(const DgradGeom& g, const DgradRoute& r, const PackA& a, const float* wfr, const float* dy, float* dx, int accumulate,
                    const DgradEpi& e, const JpCall& st) {
    const int npix = (int)g.npix, HW = g.H * g.W;
    auto go = [&](auto b) {
        main_pass(r.kind, a, wfr, 0, b, e, r.Mm, g, dy, st);
        if (!r.tail) return;
        PackA at{a.wp + (size_t)r.Mm * g.Cp, g.Cin, g.Kp, g.Cp, g.KK()};
        DgradEpi et{dx + (size_t)r.Mm * HW, g.Cin, HW, accumulate};
        launch_auto(at, b, et, r.tail, npix, g.Kp, 1, g.Kp, st);
    };
    JP_KH_SWITCH(g.KH, {
        if (g.stride == 1) go(DgradBT<KH_, true>{dy, g.Cp, npix, g.H, g.W, g.Cout, g.OH, g.OW, g.stride, g.pad, g.reflect()});
        else go(DgradBT<KH_>{dy, g.Cp, npix, g.H, g.W, g.Cout, g.OH, g.OW, g.stride, g.pad, g.reflect()});
    });
    return JP_OK;
}
// DG_SPLIT_SCRATCH / DG_SPLIT_ATOMIC
static int run_split(const DgradGeom& g, const DgradRoute& r, const PackA& a, const float* dy, float* dx, int accumulate, float* split_ws,
                     const JpCall& st) {
    const int npix = (int)g.npix, HW = g.H * g.W;
    const bool scratch = r.kind == DG_SPLIT_SCRATCH;
    if (!scratch && !accumulate) JP_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)npix * g.Cin, st));
    JP_KH_SWITCH(g.KH, {
        DgradBT<KH_> b{dy, g.Cp, npix, g.H, g.W, g.Cout, g.OH, g.OW, g.stride, g.pad, g.reflect()};
        if (scratch) launch_auto(a, b, WgradEpiWS{split_ws, g.Cin, npix}, g.Cin, npix, g.Kp, r.sl.n, r.sl.kps, st);
        else launch_auto(a, b, AtomicEpi{dx, g.Cin, HW}, g.Cin, npix, g.Kp, r.sl.n, r.sl.kps, st);
    });
    if (scratch) slice_reduce_nchw(split_ws, dx, nullptr, g.Cin, npix, HW, r.sl.n, JP_ACT_NONE, accumulate, st);
    return JP_OK;
}
static void run_p9s2d(const DgradGeom& g, int bmt, const float* wfr, const float* dy, const DgradEpi& e, const JpCall& st) {
    const int N = g.N, Cin = g.Cin, Cout = g.Cout, OH = g.OH, OW = g.OW, NST = Cout / 16;
    const unsigned* wq = reinterpret_cast<const unsigned*>(wfr);
    const float* xam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * OH * OW, st) : nullptr;
    jp_prof_before(bmt == 64 ? p9s2d_tag<1, 4, DgradEpi>() : p9s2d_tag<2, 2, DgradEpi>(), JP_NPROD * 2.0 * Cin * (double)N * OH * OW * 9.0 * Cout,
                   st);
    if (bmt == 64)
        hipLaunchKernelGGL((jp_igemm_p9s2d_kernel<1, 4, 2, DgradEpi>), dim3(4 * N * (OH / 8) * (OW / 32), 1, 1), dim3(256), 0, st, wq, dy, e,
                           Cin, Cout, NST, OH, OW, xam);
    else
        hipLaunchKernelGGL((jp_igemm_p9s2d_kernel<2, 2, 2, DgradEpi>), dim3(4 * N * (OH / 4) * (OW / 32), jp_cdiv(Cin, 128), 1), dim3(256), 0,
                           st, wq, dy, e, Cin, Cout, NST, OH, OW, xam);
    jp_prof_after(st);
}
static int run_channel_major(const DgradGeom& g, const float* dy, const float* w, const DgradEpi& e, const JpCall& st) {
    const int K = g.Cout * g.KK(), npix = (int)g.npix;
    JP_KH_SWITCH(g.KH, {
        DgradA<KH_> a{w, g.Cin, K};
        DgradB<KH_> b{dy, K, npix, g.H, g.W, g.Cout, g.OH, g.OW, g.stride, g.pad, g.reflect()};
        launch_auto(a, b, e, g.Cin, npix, K, 1, jp_cdiv(K, KC) * KC, st);
    });
    return JP_OK;
}

extern "C" int jp_conv2d_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int H, int W, int Cout,
                               int KH, int stride, int pad, int pad_mode, int accumulate, float* ws, int ws_state,
                               float* split_ws, const float* amax_dy, float* amax_dx, int* amax_dx_done, float* amax_ws,
                               void* stream) {
    if (amax_dx_done) *amax_dx_done = 0;
    JP_CHECK_ARG(dy && w && dx, "conv2d_dgrad: null pointer");
    JP_CHECK_ARG(!(pad_mode == JP_PAD_REFLECT && !(KH == 3 && stride == 1 && pad == 1 && H >= 2 && W >= 2)),
                 "conv2d_dgrad: reflect mode supports 3x3 stride 1 pad 1 only");
    const DgradGeom g = dgrad_geom(N, Cin, H, W, Cout, KH, stride, pad, pad_mode, ws != nullptr, split_ws != nullptr);
    JP_CHECK_ARG(g.npix < (1L << 31), "conv2d_dgrad: tensor too large");
    JP_CHECK_ARG(JP_NS != 2 || amax_ws || amax_dy, "conv2d_dgrad"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(dy, amax_dy);
    ax.ws = amax_ws;
    // amax_dx: folded in by the patch kernels' epilogue (+ the border fold of reflection layers); a layer with a short row tail is
    // finished by a second launch that does not report, so the slot is not offered there
    if (!g.tail()) ax.out = reinterpret_cast<unsigned*>(amax_dx);
    const JpAmaxDone done_flag{amax_dx_done, &ax};
    const JpCall st((hipStream_t)stream, &ax);
    const DgradRoute r = dgrad_route(g);
    const int OH = g.OH, OW = g.OW, Cp = g.Cp, npix = (int)g.npix;
    float* wfr = ws ? ws + dgrad_tap_floats(Cin, Cout, KH) : nullptr;       // the fragment-order pack sits behind the tap-major one
    if (!ws_state) {
        if (r.pack_tap) pack_weights(w, ws, Cout, Cin, g.KK(), Cp, 1, st);
        if (r.frag_bmt) pack_p9(w, wfr, Cout, Cin, 1, r.frag_bmt, r.frag_khw, st);
    }
    const PackA a{ws, Cin, g.Kp, Cp, g.KK()};
    const DgradEpi e{dx, Cin, H * W, accumulate};
    int rc = JP_OK;
    switch (r.kind) {
        case DG_C16: rc = jp_c16_dgrad(dy, w, dx, 0, N, Cin, Cout, H, W, accumulate, st); break;
        case DG_P9S2D: run_p9s2d(g, r.frag_bmt, wfr, dy, e, st); break;
        case DG_P1S2: {
            DgradS2PointEpi ep{dx, Cin, OH * OW, OW, accumulate};
            launch_p9s<false, false, DgradS2PointEpi, 1>(wfr, dy, ep, Cin, Cout, N, OH, OW, st, 0, r.frag_bmt);
        } break;
        case DG_S2_PARITY: {
            const int Nc = (int)g.Nc();
            PackAS2 a2{ws, Cin, Cp, Nc};
            DgradS2B b2{dy, Cp, Nc, H / 2, W / 2, Cout, OH, OW};
            DgradS2Epi e2{dx, Cin, Nc, H / 2, W / 2, accumulate};
            launch_auto(a2, b2, e2, Cin, npix, 4 * Cp, 1, 4 * Cp, st);
        } break;
        case DG_P9SM:
            jp_p9sm_launch(r.sm, wfr, dy, dx, nullptr, JP_ACT_NONE, accumulate, split_ws, Cin, Cout, N, H, W, g.KK(), 0, 1, st);
            if (r.sm.splits > 1) slice_reduce_nchw(split_ws, dx, nullptr, Cin, npix, H * W, r.sm.splits, JP_ACT_NONE, accumulate, st);
            break;
        case DG_SPLIT_SCRATCH:
        case DG_SPLIT_ATOMIC: rc = run_split(g, r, a, dy, dx, accumulate, split_ws, st); break;
        case DG_P1: launch_p1(wfr, dy, e, Cin, Cout, N, H, W, st); break;
        case DG_P9:
        case DG_ROW_TILE:
        case DG_TAP: rc = run_rows(g, r, a, wfr, dy, dx, accumulate, e, st); break;
        case DG_CHANNEL_MAJOR: rc = run_channel_major(g, dy, w, e, st); break;
        default:      // (dgrad_src3_route's kinds)
            jp_set_last_error("conv2d_dgrad: internal: not a kind of dgrad_route");
            rc = JP_EBADARG;
            break;
    }
    if (rc) return rc;
    if (r.border) border_pass(a, dy, dx, Cin, g, r.ring, split_ws, st);      // fold the reflected ring back in (border-adjacent lines only)
    JP_LAUNCH_CHECK();
}

// ---- per-source dgrad of a conv whose input is the channel concat of up to 3 sources, one of them read through the fused
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
// scratch for jp_conv2d_dgrad_src3's `split_ws` (the rule of the queries above: it has no Cout, so both ring passes at their caps):
// the border pass of the widest full-resolution segment, the edge pass of the upsampled one over the N * (H + W) half-resolution pixels
extern "C" long jp_conv2d_dgrad_src3_split_floats(int c0, int up0, int c1, int up1, int c2, int up2, int N, int H, int W) {
    const int cm = std::max(std::max(up0 ? 0 : c0, up1 ? 0 : c1), up2 ? 0 : c2);
    const int cu = std::max(std::max(up0 ? c0 : 0, up1 ? c1 : 0), up2 ? c2 : 0);
    return std::max((long)BORDER_RING.cap * cm * N * (2L * H + 2L * W), (long)EDGE_RING.cap * cu * N * ((long)H + W));
}

struct SegRoute {
    DgradKind kind;         // DG_NONE: no channels, or the gradient is not wanted
    int C, coff, up;        // channels, first row in the bank, read through the upsample
    RingPlan ring;          // the border pass (full resolution) or the edge pass (upsampled) behind the main pass
};
struct Src3Route {
    bool up_head;           // the whole call is the one-channel head on one upsampled source (conv_small.hip)
    bool segments;          // or one pass per source (dgrad_segments_ok); neither: the entry point refuses the shape
    SegRoute seg[3];
    int cx_up;              // channels of the upsampled source
    long split_use;
};
// g: the bank (all sources' channels); want[i]: source i's gradient buffer was given
static Src3Route dgrad_src3_route(const DgradGeom& g, const int* cs, const int* us, const bool* want) {
    Src3Route r{};
    r.up_head = up_head(cs[0], us[0], cs[1], cs[2], g.Cout, g.KH, g.stride, g.pad, g.pad_mode, g.H, g.W);
    r.segments = !r.up_head && dgrad_segments_ok(cs[0], us[0], cs[1], us[1], cs[2], us[2], g.N, g.H, g.W, g.Cout, g.KH, g.stride, g.pad, g.pad_mode);
    if (!r.segments) return r;
    const int N = g.N, H = g.H, W = g.W, Cout = g.Cout, h2 = H / 2, w2 = W / 2;
    const int bmt = p9_bmt(g.Cin, 9, p9_ptiles(N, H, W));     // M tile of the whole bank's fragment-order pack
    int coff = 0;
    for (int i = 0; i < 3; coff += cs[i++]) {
        const int C = cs[i];
        SegRoute& s = r.seg[i];
        s = SegRoute{DG_NONE, C, coff, us[i]};
        if (us[i]) r.cx_up = C;
        if (!C || !want[i]) continue;
        if (us[i]) {
            // split-product patch kernel over the full-resolution dY (igemm_p9sd.h), or the 16 (class, slot) GEMMs of DgradUPB
            const bool sd = p9sd_enabled() && h2 % 4 == 0 && w2 % 32 == 0 && Cout % 16 == 0 && (long)N * Cout * H * W * 4 < (1L << 31) &&
                            (long)jp_cdiv(C, 128) * N * (h2 / 4) * (w2 / 32) >= 192;
            s.kind = sd ? DG_P9SD : DG_UP_TAP;
            s.ring = edge_plan(g, C);
            r.split_use = std::max(r.split_use, ring_floats(s.ring, C, g.ring(h2, w2)));
            continue;
        }
        // a few channels (the disparity channel): direct zero-pad correlation of dY with the flipped taps instead of a 64-row MFMA tile
        if (C <= 4 && (long)C * Cout * 9 * 4 <= 48 * 1024) s.kind = DG_SMALL;
        // P9 patch kernel on this segment's tiles of the whole bank's fragment-order pack
        else if (g.Cin > 64 && C > 64 && coff % bmt == 0 && p9_ok(C, Cout, N, H, W)) s.kind = DG_P9;
        else s.kind = row_tile_ok(g, C) ? DG_ROW_TILE : DG_TAP;
        s.ring = border_plan(g, C);
        r.split_use = std::max(r.split_use, ring_floats(s.ring, C, g.ring(H, W)));
    }
    return r;
}

// the segments of r, one after the other: pack (ws_state == 0), main pass, ring pass.  Packs in `ws`: the bank's tap-major pack
// [tap][ci][Cp]; behind it (+ slack) the upsampled segment's [16][Cx][Cp]; behind that (+ slack) the flipped taps of a DG_SMALL
// segment; at dgrad_tap_floats the bank's fragment-order pack, built once for all DG_P9 segments, and behind it DG_P9SD's.
// amax_dx0: max |dx0| out of the first source's passes (main patch kernel + border fold), if it is a full-resolution one.
static int run_segments(const DgradGeom& g, const Src3Route& r, const float* dy, const float* w, float* const* dxs, const int* accs,
                        float* ws, int ws_state, float* split_ws, float* amax_dx0, int* amax_dx0_done, JpAmaxCtx& ax, const JpCall& st) {
    const int N = g.N, Cin = g.Cin, H = g.H, W = g.W, Cout = g.Cout, Cp = g.Cp, Kp = g.Kp, h2 = H / 2, w2 = W / 2, KpU = 16 * Cp;
    const long np2 = (long)N * h2 * w2;
    float* wsT = ws + ((size_t)9 * Cin + 256) * Cp;
    float* wf = wsT + (16L * r.cx_up + 256) * Cp;
    float* wfr = ws + dgrad_tap_floats(Cin, Cout, 3);
    float* wsd = wfr + p9_alloc_floats(Cin, Cp);
    const int bmt = p9_bmt(Cin, 9, p9_ptiles(N, H, W));
    if (!ws_state) pack_weights(w, ws, Cout, Cin, 9, Cp, 1, st);
    const DgradBT<3, true> b{dy, Cp, (int)g.npix, H, W, Cout, H, W, 1, 1, 1};
    bool frag_packed = false;
    for (int i = 0; i < 3; ++i) {
        const SegRoute& s = r.seg[i];
        if (s.kind == DG_NONE) continue;
        const int C = s.C, coff = s.coff;
        float* dx = dxs[i];
        ax.out = (i == 0 && !s.up) ? reinterpret_cast<unsigned*>(amax_dx0) : nullptr;
        ax.out_taken = false;
        const PackA a = s.up ? PackA{wsT, C, KpU, Cp, 16} : PackA{ws + (size_t)coff * Cp, Cin, Kp, Cp, 9};
        const DgradEpi e{dx, C, s.up ? h2 * w2 : H * W, accs[i]};
        if (!ws_state) switch (s.kind) {
            case DG_SMALL: do_pack(PACK_FLIP, w, wf, (long)C * Cout * 9, Cout, Cin, coff, C, 0, 0, st); break;
            case DG_P9:
                if (!frag_packed) pack_p9(w, wfr, Cout, Cin, 1, bmt, 9, st);
                frag_packed = true;
                break;
            case DG_P9SD:
            case DG_UP_TAP:     // (the edge pass reads the [16][Cx][Cp] pack behind either)
                do_pack(PACK_UP_DGRAD, w, wsT, 16L * C * Cp, Cout, Cin, coff, C, Cp, 0, st);
                if (s.kind == DG_P9SD) do_pack(PACK_SPLITUPD, w, wsd, p9sd_floats(C, Cout), Cout, Cin, coff, C, 0, 0, st);
                break;
            default: break;
        }
        int rc = JP_OK;
        switch (s.kind) {
            case DG_SMALL:      // (the reflection fold still comes from the border pass)
                rc = jp_conv_small_fwd(dy, Cout, 0, nullptr, 0, 0, nullptr, 0, 0, wf, nullptr, dx, N, H, W, C, JP_ACT_NONE, 0, st, accs[i]);
                break;
            case DG_P9:
            case DG_ROW_TILE:
            case DG_TAP: main_pass(s.kind, a, wfr, coff / bmt, b, e, C, g, dy, st); break;
            case DG_P9SD: {     // its pack sits behind the P9 one
                const float* xam = JP_NS == 2 ? jp_amax_of(dy, (long)N * Cout * H * W, st) : nullptr;
                jp_prof_before(p9sd_tag<DgradEpi>(), JP_NPROD * 2.0 * C * (double)np2 * 16.0 * Cp, st);
                dim3 grid(N * (h2 / 4) * (w2 / 32), jp_cdiv(C, 128), 1);
                hipLaunchKernelGGL((jp_igemm_p9sd_kernel<DgradEpi>), grid, dim3(256), 0, st, reinterpret_cast<const unsigned*>(wsd), dy, e,
                                   C, Cout, Cp / 16, h2, w2, xam);
                jp_prof_after(st);
            } break;
            case DG_UP_TAP: launch_auto(a, DgradUPB{dy, (int)np2, h2, w2, Cout}, e, C, (int)np2, KpU, 1, KpU, st); break;
            default:
                jp_set_last_error("conv2d_dgrad_src3: internal: not a kind of dgrad_src3_route");
                rc = JP_EBADARG;
                break;
        }
        if (rc) return rc;
        if (s.up) {
            edge_pass(a, dy, dx, C, g, s.ring, split_ws, st);
        } else {
            border_pass(a, dy, dx, C, g, s.ring, split_ws, st);
            if (i == 0 && amax_dx0_done) *amax_dx0_done = ax.out_taken ? 1 : 0;
        }
    }
    return JP_OK;
}

// split_ws: optional scratch of jp_conv2d_dgrad_src3_split_floats floats for the ring passes (NULL: read-modify-write epilogue)
extern "C" int jp_conv2d_dgrad_src3(const float* dy, const float* w, float* dx0, int c0, int up0, int acc0, float* dx1,
                                    int c1, int up1, int acc1, float* dx2, int c2, int up2, int acc2, int N, int H, int W,
                                    int Cout, int KH, int stride, int pad, int pad_mode, float* ws, int ws_state,
                                    float* split_ws, const float* amax_dy, float* amax_dx0, int* amax_dx0_done, float* amax_ws,
                                    void* stream) {
    if (amax_dx0_done) *amax_dx0_done = 0;
    JP_CHECK_ARG(dy && w, "conv2d_dgrad_src3: null pointer");
    float* const dxs[3] = {dx0, dx1, dx2};
    const int cs[3] = {c0, c1, c2}, us[3] = {up0, up1, up2}, accs[3] = {acc0, acc1, acc2};
    const bool want[3] = {dx0 != nullptr, dx1 != nullptr, dx2 != nullptr};
    const DgradGeom g = dgrad_geom(N, c0 + c1 + c2, H, W, Cout, KH, stride, pad, pad_mode, ws != nullptr, split_ws != nullptr);
    const Src3Route r = dgrad_src3_route(g, cs, us, want);
    JP_CHECK_ARG(r.up_head || ws != nullptr, "conv2d_dgrad_src3: null scratch");
    JP_CHECK_ARG(r.up_head || r.segments, "conv2d_dgrad_src3: shape not supported (check jp_conv2d_dgrad_src3_ok)");
    JP_CHECK_ARG(r.up_head || JP_NS != 2 || amax_ws || amax_dy, "conv2d_dgrad_src3"": every operand magnitude (amax_*) or amax_ws (jp_conv2d_amax_ws_floats floats of scratch) must be given");
    JpAmaxCtx ax;
    ax.know(dy, amax_dy);
    ax.ws = amax_ws;
    const JpCall st((hipStream_t)stream, &ax);
    int rc = JP_OK;
    if (!r.up_head) rc = run_segments(g, r, dy, w, dxs, accs, ws, ws_state, split_ws, amax_dx0, amax_dx0_done, ax, st);
    else if (dx0) rc = jp_up_head_dgrad(dy, w, dx0, N, c0, H / 2, W / 2, acc0, st);
    if (rc) return rc;
    JP_LAUNCH_CHECK();
}

