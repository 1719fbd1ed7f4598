// What conv_fwd.hip and conv_dgrad.hip share: the launch layer of the patch kernels.  Belongs here: a definition both directions
// use, or one that a function both directions call needs -- the packed-weight A loader and the row-tile B loader (forward
// instantiates REV = false, dgrad REV = true), the atomic split-K epilogue, the environment switches read by both, the tile and
// pack sizing (jp_conv2d_ws_floats sizes both directions' packs with it), launch_r3 / launch_p9s / launch_p9 / launch_p1 with
// their profiler tags, and the small-grid / small-map split policies.  Does not belong here: anything only one direction uses
// (its loaders, epilogues, tags, switches and kernel headers stay in that direction's unit), and anything wgrad needs as well
// (conv_common.h).  Of the kernel headers only those whose kernels the launchers here launch are included.
// In an anonymous namespace or inline, as in conv_common.h; not part of the ABI.  conv_fwd.hip's head has the GEMM shapes.
#pragma once
#include "conv_common.h"
#include "conv_pack.h"
#include "igemm_p9.h"
#include "igemm_p9s.h"
#include "conv_p9sm.h"
#if JP_NS == 3
#include "igemm_p1l.h"      // the persistent 1x1 kernel exists in the six-product build only (opt-in there, JP_P1L=1)
#endif
#include "scale.h"
constexpr double JP_NPROD = JP_NS == 2 ? 3.0 : 6.0;     // matrix-pipe products per fp32 product of the P9S-family kernels
#include <algorithm>
#include <cstdlib>

namespace {

// Masked-out gathers read this word instead of branching around the load: the gather stays a straight run of
// unconditional global loads (no exec-mask save/restore per element).
__device__ float jp_zero_word[4] = {0.f, 0.f, 0.f, 0.f};

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
inline long p9sd_floats(int rows, int Cout) { return (long)jp_cdiv(rows, 128) * ((long)((Cout + 31) / 32 * 2) * 16 + P9S_AHEAD) * (JP_NS * 1024) + JP_PACK_HDR; }
// P9S2D (igemm_p9s2d.h): class-uniform split-bf16 dgrad of the 3x3 stride-2 layers; JP_P9S2=0 keeps the generic DgradS2B form
inline bool p9s2_enabled() {
    static const bool on = [] { const char* e = getenv("JP_P9S2"); return !(e && e[0] == '0'); }();
    return on;
}
// per-kernel switches below JP_P9S2 (A/B and bisection): JP_P9S2D / JP_P9S2F / JP_P1S2 / JP_P7S = 0 keep the generic engine
#define JP_ENV_ON(NAME) ([] { static const bool on = [] { const char* e = getenv(NAME); return !(e && e[0] == '0'); }(); return on; }())
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
inline bool p1s2_ok(int rows, int red, int N, int OH, int OW) {
    const int tr = rows <= 64 ? 8 : 4;
    return p9s_enabled() && p9s2_enabled() && JP_ENV_ON("JP_P1S2") && rows >= 32 && red >= 64 && red % 64 == 0 && OW % 32 == 0 && OH % tr == 0 &&
           (long)N * red * OH * OW * 16 < (1L << 31) &&
           (long)jp_cdiv(rows, p9_bmt(rows, 1, p9_ptiles(N, OH, OW))) * N * (OH / tr) * (OW / 32) >= 192;
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

}  // namespace

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

#pragma GCC visibility push(hidden)
// deterministic small-grid split-K fold (slice_reduce_nchw_kernel): defined in conv_fwd.hip, launched by both directions
void slice_reduce_nchw(const float* part, float* y, const float* bias, int M, int Npix, int HW, int splits, int act, int accumulate,
                       hipStream_t st);
#pragma GCC visibility pop
