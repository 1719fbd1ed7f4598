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

// floats of jp_conv2d_dgrad's optional `split_ws` (as jp_conv2d_fwd_split_floats, conv_fwd.hip, for the forward)
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
