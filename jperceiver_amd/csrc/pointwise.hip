// HBM-bound streaming kernels of the train step: max-pools (3x3 s2 p1 resnet.py:94, 5x5 s1 p2
// layers.py:191, 2x2 layout_model.py:84), nearest 2x upsample (layers.py:110), channel concat /
// split, dropout-mask multiply (depth_decoder.py:52-53), activation backward, adds, bilinear and
// area resizes (net.py:632,692,762).  NCHW fp32; one thread per output element, lanes along W so
// every wave touches contiguous 256-B segments.
#include "jp_common.h"
#include "bilinear.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;
inline int blocks_for(long n) { return (int)std::min<long>((n + TPB - 1) / TPB, 1 << 20); }

// ------------------------------------------------------------------ max pool
// idx stores the window-relative argmax (ky*k+kx) of the first maximum in scan order
// (PyTorch: `val > max || isnan(val)` -> first max wins), so backward is a gather without atomics.
constexpr int MP_TW = 64, MP_TH = 8;   // output (fwd) / input (bwd) tile per workgroup

// LDS-tiled: the input patch of a 64x8 output tile is staged once (coalesced rows, -inf outside the image),
// then every output scans its k x k window from LDS.  grid (tiles_x, tiles_y, planes)
__global__ __launch_bounds__(TPB) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ idx, int H, int W, int OH, int OW,
                                                          int k, int s, int p) {
    extern __shared__ float tile[];
    const size_t nc = blockIdx.z;
    const float* xp = x + nc * H * W;
    const int ox0 = blockIdx.x * MP_TW, oy0 = blockIdx.y * MP_TH;
    const int pw = (MP_TW - 1) * s + k, ph = (MP_TH - 1) * s + k;
    const int ix0 = ox0 * s - p, iy0 = oy0 * s - p;
    for (int i = threadIdx.x; i < pw * ph; i += TPB) {
        const int ly = i / pw, lx = i - ly * pw;
        const int iy = iy0 + ly, ix = ix0 + lx;
        tile[i] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? xp[iy * W + ix] : -INFINITY;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < MP_TW * MP_TH; o += TPB) {
        const int ty = o / MP_TW, tx = o - ty * MP_TW;
        const int oy = oy0 + ty, ox = ox0 + tx;
        if (oy >= OH || ox >= OW) continue;
        float best = -INFINITY;
        int bi = -1;
        for (int ky = 0; ky < k; ++ky) {
            const float* row = tile + (ty * s + ky) * pw + tx * s;
            const bool rin = (unsigned)(iy0 + ty * s + ky) < (unsigned)H;
            for (int kx = 0; kx < k; ++kx) {
                const float v = row[kx];
                const bool in = rin && (unsigned)(ix0 + tx * s + kx) < (unsigned)W;
                // PyTorch: first element in scan order with (val > max) || isnan(val); padding never wins
                if (in && (bi < 0 || v > best || v != v)) { best = v; bi = ky * k + kx; }
            }
        }
        y[nc * OH * OW + oy * OW + ox] = best;
        idx[nc * OH * OW + oy * OW + ox] = (uint8_t)max(bi, 0);
    }
}

// gather-form backward over a 64x8 INPUT tile: the covering dy / argmax patch is staged in LDS
__global__ __launch_bounds__(TPB) void maxpool_bwd_kernel(const float* __restrict__ dy,
                                                          const uint8_t* __restrict__ idx, float* __restrict__ dx,
                                                          const float* __restrict__ addend, int H, int W, int OH,
                                                          int OW, int k, int s, int p, int pw, int ph) {
    extern __shared__ float tile[];           // [ph*pw] dy  then  [ph*pw] idx (as int)
    int* itile = reinterpret_cast<int*>(tile + pw * ph);
    const size_t nc = blockIdx.z;
    const float* dp = dy + nc * OH * OW;
    const uint8_t* ip = idx + nc * OH * OW;
    const int ix0 = blockIdx.x * MP_TW, iy0 = blockIdx.y * MP_TH;
    // first output row/col that can cover the tile's first input row/col
    int oy0 = iy0 + p - k + 1;
    oy0 = oy0 <= 0 ? 0 : (oy0 + s - 1) / s;
    int ox0 = ix0 + p - k + 1;
    ox0 = ox0 <= 0 ? 0 : (ox0 + s - 1) / s;
    for (int i = threadIdx.x; i < pw * ph; i += TPB) {
        const int ly = i / pw, lx = i - ly * pw;
        const int oy = oy0 + ly, ox = ox0 + lx;
        const bool in = oy < OH && ox < OW;
        tile[i] = in ? dp[oy * OW + ox] : 0.f;
        itile[i] = in ? (int)ip[oy * OW + ox] : -1;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < MP_TW * MP_TH; o += TPB) {
        const int ty = o / MP_TW, tx = o - ty * MP_TW;
        const int iy = iy0 + ty, ix = ix0 + tx;
        if (iy >= H || ix >= W) continue;
        int oy_lo = iy + p - k + 1;
        oy_lo = oy_lo <= 0 ? 0 : (oy_lo + s - 1) / s;
        const int oy_hi = min(OH - 1, (iy + p) / s);
        int ox_lo = ix + p - k + 1;
        ox_lo = ox_lo <= 0 ? 0 : (ox_lo + s - 1) / s;
        const int ox_hi = min(OW - 1, (ix + p) / s);
        float g = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const int ky = iy - (oy * s - p);
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const int kx = ix - (ox * s - p);
                const int li = (oy - oy0) * pw + (ox - ox0);
                if (itile[li] == ky * k + kx) g += tile[li];
            }
        }
        if (addend) g += addend[nc * H * W + iy * W + ix];
        dx[nc * H * W + iy * W + ix] = g;
    }
}

// Compile-time (K, S) forward: 64x16 output tile, every thread owns 4 vertically adjacent outputs of one column so a
// staged row is read once from LDS and feeds all the windows that contain it (rows arrive in scan order, so the
// first-maximum rule is preserved).  Padding is staged as -inf and therefore never wins.
constexpr int MPF_TH = 16;
template <int K, int S>
__global__ __launch_bounds__(TPB) void maxpool_fwd_t_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            uint8_t* __restrict__ idx, int H, int W, int OH, int OW,
                                                            int p) {
    constexpr int PW = (MP_TW - 1) * S + K, PH = (MPF_TH - 1) * S + K;
    __shared__ float tile[PW * PH];
    const size_t nc = blockIdx.z;
    const float* xp = x + nc * H * W;
    const int ox0 = blockIdx.x * MP_TW, oy0 = blockIdx.y * MPF_TH;
    const int ix0 = ox0 * S - p, iy0 = oy0 * S - p;
    for (int i = threadIdx.x; i < PW * PH; i += TPB) {
        const int ly = i / PW, lx = i - ly * PW;
        const int iy = iy0 + ly, ix = ix0 + lx;
        tile[i] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? xp[iy * W + ix] : -INFINITY;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
    float best[4];
    int bi[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { best[j] = -INFINITY; bi[j] = 0; }
    const float* base = tile + (q * 4 * S) * PW + tx * S;
    constexpr int R = 3 * S + K;
    // separable with the scan-order tie rule kept: per staged row the first maximum over kx (once, shared by the up
    // to K/S windows that contain the row), then per window the first maximum over ky of those row results
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float rv = base[r * PW];
        int rk = 0;
#pragma unroll
        for (int kx = 1; kx < K; ++kx) {
            const float v = base[r * PW + kx];
            const bool take = v > rv || v != v;     // PyTorch's rule: first maximum, a NaN always takes over
            rv = take ? v : rv;
            rk = take ? kx : rk;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ky = r - j * S;
            if (ky < 0 || ky >= K) continue;
            const bool take = ky == 0 || rv > best[j] || rv != rv;
            best[j] = take ? rv : best[j];
            bi[j] = take ? ky * K + rk : bi[j];
        }
    }
    const int ox = ox0 + tx;
    if (ox >= OW) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + q * 4 + j;
        if (oy < OH) {
            y[nc * OH * OW + oy * OW + ox] = best[j];
            idx[nc * OH * OW + oy * OW + ox] = (uint8_t)bi[j];
        }
    }
}

// Compile-time K, stride 1 backward: 64x16 input tile, the covering (dy, argmax) patch staged with -1 outside the
// output, so the K*K candidate scan needs no bounds tests.
template <int K>
__global__ __launch_bounds__(TPB) void maxpool_bwd_s1_kernel(const float* __restrict__ dy,
                                                             const uint8_t* __restrict__ idx, float* __restrict__ dx,
                                                             const float* __restrict__ addend, int H, int W, int OH,
                                                             int OW, int p) {
    constexpr int PW = MP_TW + K - 1, PH = MPF_TH + K - 1;
    __shared__ float tile[PW * PH];
    __shared__ int itile[PW * PH];
    const size_t nc = blockIdx.z;
    const float* dp = dy + nc * OH * OW;
    const uint8_t* ip = idx + nc * OH * OW;
    const int ix0 = blockIdx.x * MP_TW, iy0 = blockIdx.y * MPF_TH;
    const int oy0 = iy0 + p - (K - 1), ox0 = ix0 + p - (K - 1);
    for (int i = threadIdx.x; i < PW * PH; i += TPB) {
        const int ly = i / PW, lx = i - ly * PW;
        const int oy = oy0 + ly, ox = ox0 + lx;
        const bool in = (unsigned)oy < (unsigned)OH && (unsigned)ox < (unsigned)OW;
        tile[i] = in ? dp[oy * OW + ox] : 0.f;
        itile[i] = in ? (int)ip[oy * OW + ox] : -1;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int ix = ix0 + tx;
    if (ix >= W) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ty = q * 4 + j, iy = iy0 + ty;
        if (iy >= H) break;
        float g = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int li = (ty + K - 1 - ky) * PW + tx + K - 1 - kx;
                g += itile[li] == ky * K + kx ? tile[li] : 0.f;
            }
        if (addend) g += addend[nc * H * W + iy * W + ix];
        dx[nc * H * W + iy * W + ix] = g;
    }
}

// ------------------------------------------------------------------ 5x5 stride-1 pad-2 max pool, row-streaming form
// The CRP chains (layers.py:184-199) pool 256-channel maps of width 32 ... 256.  For W = 4*L with L | 64 a GROUP of L
// lanes owns whole image rows (one float4 per lane = 16-B coalesced accesses, the row's left / right neighbours are
// the adjacent lanes: wave shuffles, no LDS tile, no barrier) and walks down a band of rows with a 5-row register
// window.  Both passes are separable with the scan-order (first maximum) tie rule kept:
//   forward : per row the first maximum over kx of each column's 5 taps (rv, rk), then per output the first maximum
//             over ky of the 5 row results;  idx = ky*5 + rk[that row].
//   backward: rk of a row does not depend on the window that picked the row, so the gather splits the same way:
//             t[r][ox] = sum over ky of dy[r+2-ky][ox] where that window picked row r, then dx[r][x] = sum over the 5
//             columns ox whose row pick points at x.  10 candidates per input instead of 25 (+ the fused residual addend).
// grid: ceil(units / (4*G)) blocks of 4 waves, G = 64/L groups per wave, unit = (plane, band of RB rows).
template <int L>
__device__ __forceinline__ void row5_neighbours(const float4 v, int lane_in_row, float e[8], float pad) {
    // e[0..7] = columns 4*lane-2 .. 4*lane+5
    const float lz = __shfl_up(v.z, 1, 64), lw = __shfl_up(v.w, 1, 64);
    const float rx = __shfl_down(v.x, 1, 64), ry = __shfl_down(v.y, 1, 64);
    e[0] = lane_in_row == 0 ? pad : lz;
    e[1] = lane_in_row == 0 ? pad : lw;
    e[2] = v.x; e[3] = v.y; e[4] = v.z; e[5] = v.w;
    e[6] = lane_in_row == L - 1 ? pad : rx;
    e[7] = lane_in_row == L - 1 ? pad : ry;
}

template <int L>
__global__ __launch_bounds__(TPB) void maxpool5_rows_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                uint8_t* __restrict__ idx, int NC, int H, int RB, int bands) {
    constexpr int G = 64 / L, W = 4 * L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / L, lir = lane % L;
    const long unit = ((long)blockIdx.x * 4 + wave) * G + grp;
    const bool live = unit < (long)NC * bands;
    const long nc = live ? unit / bands : 0;
    const int r0 = live ? (int)(unit % bands) * RB : 0;
    const int r1 = min(H, r0 + RB);                       // output rows [r0, r1)
    const float4* xp = reinterpret_cast<const float4*>(x + nc * (long)H * W) + lir;
    float4* yp = reinterpret_cast<float4*>(y + nc * (long)H * W) + lir;
    uchar4* ip = reinterpret_cast<uchar4*>(idx + nc * (long)H * W) + lir;
    const float NEG = -INFINITY;
    float rv[5][4];
    int rk[5][4];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { rv[i][j] = NEG; rk[i][j] = 0; }
    const int rend = live ? r1 + 2 : r0 - 2;             // dead groups still execute the shuffles of their wave: run 0 rows
    for (int r = r0 - 2; r < rend; ++r) {
        float4 v = make_float4(NEG, NEG, NEG, NEG);
        if ((unsigned)r < (unsigned)H) v = xp[(long)r * L];
        float e[8];
        row5_neighbours<L>(v, lir, e, NEG);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { rv[i][j] = rv[i + 1][j]; rk[i][j] = rk[i + 1][j]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                    // first maximum over kx (a NaN always takes over: PyTorch's rule)
            float b = e[j];
            int k = 0;
#pragma unroll
            for (int kx = 1; kx < 5; ++kx) {
                const float c = e[j + kx];
                const bool take = c > b || c != c;
                b = take ? c : b;
                k = take ? kx : k;
            }
            rv[4][j] = b;
            rk[4][j] = k;
        }
        const int oy = r - 2;
        if (oy >= r0) {                                  // rows oy-2 .. oy+2 are in the window: first maximum over ky
            float o[4];
            unsigned char oi[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float b = rv[0][j];
                int bi = rk[0][j];
#pragma unroll
                for (int ky = 1; ky < 5; ++ky) {
                    const float c = rv[ky][j];
                    const bool take = c > b || c != c;
                    b = take ? c : b;
                    bi = take ? ky * 5 + rk[ky][j] : bi;
                }
                o[j] = b;
                oi[j] = (unsigned char)bi;
            }
            yp[(long)oy * L] = make_float4(o[0], o[1], o[2], o[3]);
            ip[(long)oy * L] = make_uchar4(oi[0], oi[1], oi[2], oi[3]);
        }
    }
}

template <int L>
__global__ __launch_bounds__(TPB) void maxpool5_rows_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                                float* __restrict__ dx, const float* __restrict__ addend,
                                                                int NC, int H, int RB, int bands, unsigned* __restrict__ amax) {
    constexpr int G = 64 / L, W = 4 * L;
    float mx = 0.f;                                       // largest stored magnitude (the next dgrad's operand scale)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / L, lir = lane % L;
    const long unit = ((long)blockIdx.x * 4 + wave) * G + grp;
    const bool live = unit < (long)NC * bands;
    const long nc = live ? unit / bands : 0;
    const int r0 = live ? (int)(unit % bands) * RB : 0;
    const int r1 = min(H, r0 + RB);                       // input rows [r0, r1)
    const float4* dp = reinterpret_cast<const float4*>(dy + nc * (long)H * W) + lir;
    const uchar4* ip = reinterpret_cast<const uchar4*>(idx + nc * (long)H * W) + lir;
    const float4* ap = addend ? reinterpret_cast<const float4*>(addend + nc * (long)H * W) + lir : nullptr;
    float4* op = reinterpret_cast<float4*>(dx + nc * (long)H * W) + lir;
    // window of output rows oy = r-2 .. r+2 around input row r: gradient, picked row (ky) and picked column (kx)
    float d[5][4];
    int wy[5][4], wx[5][4];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[i][j] = 0.f; wy[i][j] = 7; wx[i][j] = 0; }
    const int oend = live ? r1 + 2 : r0 - 2;
    for (int oy = r0 - 2; oy < oend; ++oy) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { d[i][j] = d[i + 1][j]; wy[i][j] = wy[i + 1][j]; wx[i][j] = wx[i + 1][j]; }
        if ((unsigned)oy < (unsigned)H) {
            const float4 g = dp[(long)oy * L];
            const uchar4 q = ip[(long)oy * L];
            const float gg[4] = {g.x, g.y, g.z, g.w};
            const int qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ky = (qq[j] * 13) >> 6;         // / 5 for 0..24
                d[4][j] = gg[j];
                wy[4][j] = ky;
                wx[4][j] = qq[j] - 5 * ky;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { d[4][j] = 0.f; wy[4][j] = 7; wx[4][j] = 0; }
        }
        const int r = oy - 2;                             // window slot i holds output row r-2+i, which reaches r via ky = 4-i
        // (executed by every lane, also before the first input row: the shuffles below need the whole wave)
        float t[4];
        float tk[4];                                      // picked column as a float: travels through the same shuffles
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
            int kx = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const bool hit = wy[i][j] == 4 - i;
                acc += hit ? d[i][j] : 0.f;
                kx = hit ? wx[i][j] : kx;
            }
            t[j] = acc;
            tk[j] = (float)kx;
        }
        float et[8], ek[8];
        row5_neighbours<L>(make_float4(t[0], t[1], t[2], t[3]), lir, et, 0.f);
        row5_neighbours<L>(make_float4(tk[0], tk[1], tk[2], tk[3]), lir, ek, -1.f);
        if (r >= r0 && r < r1) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                 // input column 4*lane+j <- output columns ox = x-2 .. x+2 (e index j .. j+4)
                float acc = 0.f;
#pragma unroll
                for (int m = 0; m < 5; ++m) acc += ek[j + m] == (float)(4 - m) ? et[j + m] : 0.f;   // kx = x - ox + 2 = 4 - m
                o[j] = acc;
            }
            if (ap) { const float4 a = ap[(long)r * L]; o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w; }
            op[(long)r * L] = make_float4(o[0], o[1], o[2], o[3]);
            mx = fmaxf(fmaxf(mx, fmaxf(jp_fmag(o[0]), jp_fmag(o[1]))), fmaxf(jp_fmag(o[2]), jp_fmag(o[3])));
        }
    }
    jp_wave_amax_commit(mx, amax);
}

// ------------------------------------------------------------------ 3x3 stride-2 pad-1 max pool backward (the ResNet stem)
// Output (i, j) covers input rows 2i-1 .. 2i+1, so the 2x2 input cell (2i .. 2i+1, 2j .. 2j+1) gathers from the four outputs
// (i .. i+1, j .. j+1) only: [2i][2j] <- (i,j) tap 4;  [2i][2j+1] <- (i,j) tap 5, (i,j+1) tap 3;  [2i+1][2j] <- (i,j) tap 7,
// (i+1,j) tap 1;  [2i+1][2j+1] <- (i,j) tap 8, (i,j+1) tap 6, (i+1,j) tap 2, (i+1,j+1) tap 0.  A thread owns two output columns
// (-> one float4 of each of the two input rows) and walks down a band of RB output rows, keeping the previous output row in
// registers: dy and the argmax byte are read once, dx is written once with 16-byte stores.
__global__ __launch_bounds__(TPB) void maxpool3s2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                             float* __restrict__ dx, const float* __restrict__ addend, long units,
                                                             int OH, int OW, int RB, int bands) {
    const long u = (long)blockIdx.x * TPB + threadIdx.x;
    if (u >= units) return;
    const int OW2 = OW >> 1, W = 2 * OW;
    const int q = (int)(u % OW2);
    const long v = u / OW2;
    const int b = (int)(v % bands);
    const long nc = v / bands;
    const int i0 = b * RB, i1 = min(OH, i0 + RB);
    const float* dp = dy + nc * (long)OH * OW + 2 * q;
    const uint8_t* ip = idx + nc * (long)OH * OW + 2 * q;
    float* op = dx + nc * 4L * OH * OW + 4 * q;
    const float* ap = addend ? addend + nc * 4L * OH * OW + 4 * q : nullptr;
    const bool right = 2 * q + 2 < OW;
    float g[2][3];                 // [row parity: current / next][output columns 2q, 2q+1, 2q+2]
    int k[2][3];
    auto load = [&](int slot, int i) {
        if (i < OH) {
            const float2 a = *reinterpret_cast<const float2*>(dp + (long)i * OW);
            const uchar2 c = *reinterpret_cast<const uchar2*>(ip + (long)i * OW);
            g[slot][0] = a.x; g[slot][1] = a.y; k[slot][0] = c.x; k[slot][1] = c.y;
            g[slot][2] = right ? dp[(long)i * OW + 2] : 0.f;
            k[slot][2] = right ? (int)ip[(long)i * OW + 2] : -1;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) { g[slot][c] = 0.f; k[slot][c] = -1; }
        }
    };
    load(0, i0);
    for (int i = i0; i < i1; ++i) {
        load(1, i + 1);
        float4 r0, r1;
        // input row 2i, columns 4q .. 4q+3 (outputs of row i only)
        r0.x = k[0][0] == 4 ? g[0][0] : 0.f;
        r0.y = (k[0][0] == 5 ? g[0][0] : 0.f) + (k[0][1] == 3 ? g[0][1] : 0.f);
        r0.z = k[0][1] == 4 ? g[0][1] : 0.f;
        r0.w = (k[0][1] == 5 ? g[0][1] : 0.f) + (k[0][2] == 3 ? g[0][2] : 0.f);
        // input row 2i+1 (outputs of rows i and i+1)
        r1.x = (k[0][0] == 7 ? g[0][0] : 0.f) + (k[1][0] == 1 ? g[1][0] : 0.f);
        r1.y = (k[0][0] == 8 ? g[0][0] : 0.f) + (k[0][1] == 6 ? g[0][1] : 0.f) + (k[1][0] == 2 ? g[1][0] : 0.f) + (k[1][1] == 0 ? g[1][1] : 0.f);
        r1.z = (k[0][1] == 7 ? g[0][1] : 0.f) + (k[1][1] == 1 ? g[1][1] : 0.f);
        r1.w = (k[0][1] == 8 ? g[0][1] : 0.f) + (k[0][2] == 6 ? g[0][2] : 0.f) + (k[1][1] == 2 ? g[1][1] : 0.f) + (k[1][2] == 0 ? g[1][2] : 0.f);
        if (ap) {
            const float4 a0 = *reinterpret_cast<const float4*>(ap + (long)(2 * i) * W);
            const float4 a1 = *reinterpret_cast<const float4*>(ap + (long)(2 * i + 1) * W);
            r0.x += a0.x; r0.y += a0.y; r0.z += a0.z; r0.w += a0.w;
            r1.x += a1.x; r1.y += a1.y; r1.z += a1.z; r1.w += a1.w;
        }
        *reinterpret_cast<float4*>(op + (long)(2 * i) * W) = r0;
        *reinterpret_cast<float4*>(op + (long)(2 * i + 1) * W) = r1;
#pragma unroll
        for (int c = 0; c < 3; ++c) { g[0][c] = g[1][c]; k[0][c] = k[1][c]; }
    }
}

template <int L>
static void launch_pool5_rows(bool fwd, const float* a, float* out, uint8_t* idx, const uint8_t* cidx, const float* addend,
                              int NC, int H, hipStream_t st, unsigned* amax) {
    // band height: enough (plane, band) units for >= ~16 waves per CU (a wave has one row load in flight) -- 4 halo rows per band
    const int G = 64 / L;
    int RB = H <= 64 ? H : 64;
    while (RB > 16 && (long)NC * jp_cdiv(H, RB) / G < 4096) RB >>= 1;
    const int bands = jp_cdiv(H, RB);
    const long units = (long)NC * bands;
    const dim3 grid((unsigned)jp_cdiv(units, 4L * G));
    if (fwd) hipLaunchKernelGGL((maxpool5_rows_fwd_kernel<L>), grid, dim3(TPB), 0, st, a, out, idx, NC, H, RB, bands);
    else hipLaunchKernelGGL((maxpool5_rows_bwd_kernel<L>), grid, dim3(TPB), 0, st, a, cidx, out, addend, NC, H, RB, bands, amax);
}
static bool pool5_rows_ok(int k, int s, int p, int W) {
    return k == 5 && s == 1 && p == 2 && (W == 32 || W == 64 || W == 128 || W == 256);
}
static void pool5_rows(bool fwd, const float* a, float* out, uint8_t* idx, const uint8_t* cidx, const float* addend, int NC,
                       int H, int W, hipStream_t st, unsigned* amax = nullptr) {
    switch (W) {
        case 32: launch_pool5_rows<8>(fwd, a, out, idx, cidx, addend, NC, H, st, amax); break;
        case 64: launch_pool5_rows<16>(fwd, a, out, idx, cidx, addend, NC, H, st, amax); break;
        case 128: launch_pool5_rows<32>(fwd, a, out, idx, cidx, addend, NC, H, st, amax); break;
        default: launch_pool5_rows<64>(fwd, a, out, idx, cidx, addend, NC, H, st, amax); break;
    }
}

// ------------------------------------------------------------------ nearest 2x upsample
__global__ __launch_bounds__(TPB) void upsample2x_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             long total, int C, int H, int W, int dstC, int dc0) {
    const int OW = 2 * W, OH = 2 * H;
    for (long o = (long)blockIdx.x * TPB + threadIdx.x; o < total; o += (long)gridDim.x * TPB) {
        const int ox = (int)(o % OW);
        const long t = o / OW;
        const int oy = (int)(t % OH);
        const long nc = t / OH;
        const int c = (int)(nc % C);
        const long n = nc / C;
        y[((n * dstC + dc0 + c) * OH + oy) * OW + ox] = x[(nc * H + (oy >> 1)) * W + (ox >> 1)];
    }
}

// W % 4 == 0: one float4 of input -> two rows x two float4 of output (16-B accesses on both sides, 32-bit indexing)
__global__ __launch_bounds__(TPB) void upsample2x_fwd_v4_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                unsigned total4, int C, int H, int W4, int dstC,
                                                                int dc0) {
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total4; i += gridDim.x * TPB) {
        const unsigned xq = i % W4, t = i / W4;
        const unsigned yy = t % H, nc = t / H;
        const unsigned c = nc % C, n = nc / C;
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float4* o = reinterpret_cast<float4*>(y + (((size_t)n * dstC + dc0 + c) * (2 * H) + 2 * yy) * (8 * W4)) + 2 * xq;
        const float4 a = make_float4(v.x, v.x, v.y, v.y), b = make_float4(v.z, v.z, v.w, v.w);
        o[0] = a; o[1] = b;
        o[2 * W4] = a; o[2 * W4 + 1] = b;
    }
}

// W % 2 == 0: two input-gradient elements from two float4 rows of dy
__global__ __launch_bounds__(TPB) void upsample2x_bwd_v2_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                unsigned total2, int C, int H, int W2, int Ctot, int c0,
                                                                int accumulate) {
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total2; i += gridDim.x * TPB) {
        const unsigned xp = i % W2, t = i / W2;
        const unsigned yy = t % H, nc = t / H;
        const unsigned c = nc % C, n = nc / C;
        const float4* d = reinterpret_cast<const float4*>(dy + (((size_t)n * Ctot + c0 + c) * (2 * H) + 2 * yy) * (4 * W2)) + xp;
        const float4 r0 = d[0], r1 = d[W2];
        float2 g = make_float2(r0.x + r0.y + r1.x + r1.y, r0.z + r0.w + r1.z + r1.w);
        float2* o = reinterpret_cast<float2*>(dx) + i;
        if (accumulate) { const float2 p = *o; g.x += p.x; g.y += p.y; }
        *o = g;
    }
}

// dx[nc][y][x] = sum of the 2x2 block of dy; dy may be a channel slice of a wider tensor:
// element (n, c, y, x) lives at dy[((n*Ctot + c0 + c)*OH + y)*OW + x]
__global__ __launch_bounds__(TPB) void upsample2x_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                             long total, int C, int H, int W, int Ctot, int c0,
                                                             int accumulate) {
    const int OW = 2 * W;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int x = (int)(i % W);
        const long t = i / W;
        const int y = (int)(t % H);
        const long nc = t / H;
        const int c = (int)(nc % C);
        const long n = nc / C;
        const float* d = dy + ((n * Ctot + c0 + c) * (2L * H) + 2 * y) * OW + 2 * x;
        const float g = d[0] + d[1] + d[OW] + d[OW + 1];
        dx[i] = accumulate ? dx[i] + g : g;
    }
}

// ------------------------------------------------------------------ channel slice copy
// dst[n][dc0 + c][hw] = src[n][sc0 + c][hw]  for c < C  (concat and split are both this)
__global__ __launch_bounds__(TPB) void copy_channels_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            long total, int C, int HW, int srcC, int sc0, int dstC,
                                                            int dc0, int accumulate) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int p = (int)(i % HW);
        const long t = i / HW;
        const int c = (int)(t % C);
        const long n = t / C;
        const float v = src[(n * srcC + sc0 + c) * HW + p];
        float* q = dst + (n * dstC + dc0 + c) * HW + p;
        *q = accumulate ? *q + v : v;
    }
}

__global__ __launch_bounds__(TPB) void copy_channels_v4_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                               unsigned total4, int C, int HW4, int srcC, int sc0,
                                                               int dstC, int dc0, int accumulate) {
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total4; i += gridDim.x * TPB) {
        const unsigned p = i % HW4, t = i / HW4;
        const unsigned c = t % C, n = t / C;
        float4 v = reinterpret_cast<const float4*>(src)[((size_t)n * srcC + sc0 + c) * HW4 + p];
        float4* q = reinterpret_cast<float4*>(dst) + ((size_t)n * dstC + dc0 + c) * HW4 + p;
        if (accumulate) { const float4 o = *q; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        *q = v;
    }
}

// ------------------------------------------------------------------ elementwise
// out = alpha * a (*|+) b ...
// ---- elementwise: 16 B per lane on the 16-B aligned body (every torch allocation is >= 256-B aligned; views into the
// flat arenas are 256-B aligned slices), scalar on the tail / unaligned operands.  F: float4 lanes -> float4.
template <class F4, class F1>
__device__ __forceinline__ void ew_loop(long n, bool aligned, F4 f4, F1 f1) {
    const long n4 = aligned ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long)gridDim.x * TPB) f4(i);
    for (long i = (n4 << 2) + (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) f1(i);
}
__device__ __forceinline__ bool al16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                                     const void* e = nullptr, const void* f = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 15) == 0;
}
#define JP_F4(p) reinterpret_cast<const float4*>(p)
#define JP_F4W(p) reinterpret_cast<float4*>(p)

__global__ __launch_bounds__(TPB) void axpby_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                    float* __restrict__ out, long n, float alpha, float beta) {
    ew_loop(n, al16(a, b, out),
            [&](long i) {
                const float4 x = JP_F4(a)[i];
                float4 r = make_float4(alpha * x.x, alpha * x.y, alpha * x.z, alpha * x.w);
                if (b) { const float4 y = JP_F4(b)[i]; r.x += beta * y.x; r.y += beta * y.y; r.z += beta * y.z; r.w += beta * y.w; }
                JP_F4W(out)[i] = r;
            },
            [&](long i) { out[i] = alpha * a[i] + (b ? beta * b[i] : 0.f); });
}

// out = a0 + a1 (+ a2 + a3 + a4): the residual sum of a CRP block (layers.py:193-198) in ONE pass instead of a
// chain of pairwise adds.  Left-to-right order = the reference's accumulation order (x + top1 + top2 + ...).
__global__ __launch_bounds__(TPB) void sum_n_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                    const float* __restrict__ a2, const float* __restrict__ a3,
                                                    const float* __restrict__ a4, float* __restrict__ out, long n,
                                                    unsigned* __restrict__ amax) {
    float mx = 0.f;                      // largest |out| this thread wrote (-> amax_out: the operand scale of the convolution that reads it)
    ew_loop(n, al16(a0, a1, a2, a3, a4, out),
            [&](long i) {
                float4 r = JP_F4(a0)[i];
                const float4 b = JP_F4(a1)[i];
                r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w;
                if (a2) { const float4 c = JP_F4(a2)[i]; r.x += c.x; r.y += c.y; r.z += c.z; r.w += c.w; }
                if (a3) { const float4 c = JP_F4(a3)[i]; r.x += c.x; r.y += c.y; r.z += c.z; r.w += c.w; }
                if (a4) { const float4 c = JP_F4(a4)[i]; r.x += c.x; r.y += c.y; r.z += c.z; r.w += c.w; }
                JP_F4W(out)[i] = r;
                mx = fmaxf(fmaxf(mx, fmaxf(jp_fmag(r.x), jp_fmag(r.y))), fmaxf(jp_fmag(r.z), jp_fmag(r.w)));
            },
            [&](long i) {
                float r = a0[i] + a1[i];
                if (a2) r += a2[i];
                if (a3) r += a3[i];
                if (a4) r += a4[i];
                out[i] = r;
                mx = fmaxf(mx, jp_fmag(r));
            });
    jp_block_amax_commit(mx, amax);
}

__global__ __launch_bounds__(TPB) void mul_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, long n, float scale) {
    ew_loop(n, al16(a, b, out),
            [&](long i) {
                const float4 x = JP_F4(a)[i], y = JP_F4(b)[i];
                JP_F4W(out)[i] = make_float4(x.x * y.x * scale, x.y * y.y * scale, x.z * y.z * scale, x.w * y.w * scale);
            },
            [&](long i) { out[i] = a[i] * b[i] * scale; });
}

__global__ __launch_bounds__(TPB) void affine_kernel(const float* __restrict__ a, float* __restrict__ out, long n,
                                                     float scale, float shift) {
    ew_loop(n, al16(a, out),
            [&](long i) {
                const float4 x = JP_F4(a)[i];
                JP_F4W(out)[i] = make_float4(x.x * scale + shift, x.y * scale + shift, x.z * scale + shift, x.w * scale + shift);
            },
            [&](long i) { out[i] = a[i] * scale + shift; });
}

__global__ __launch_bounds__(TPB) void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n,
                                                      int act) {
    ew_loop(n, al16(x, y),
            [&](long i) {
                const float4 v = JP_F4(x)[i];
                JP_F4W(y)[i] = make_float4(jp_act(v.x, act), jp_act(v.y, act), jp_act(v.z, act), jp_act(v.w, act));
            },
            [&](long i) { y[i] = jp_act(x[i], act); });
}

// dx = dy * act'(.) expressed through the activation OUTPUT y (valid for relu / leaky / sigmoid)
__device__ __forceinline__ float act_bwd1(float d, float v, int act) {
    if (act == JP_ACT_RELU) return v > 0.f ? d : 0.f;
    if (act == JP_ACT_LEAKY) return v > 0.f ? d : 0.01f * d;
    if (act == JP_ACT_SIGMOID) return d * v * (1.f - v);
    return d;
}
__global__ __launch_bounds__(TPB) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      float* __restrict__ dx, long n, int act, unsigned* __restrict__ amax) {
    float mx = 0.f;                      // largest |dx| this thread wrote (-> amax_dx)
    ew_loop(n, al16(dy, y, dx),
            [&](long i) {
                const float4 d = JP_F4(dy)[i], v = JP_F4(y)[i];
                const float4 o = make_float4(act_bwd1(d.x, v.x, act), act_bwd1(d.y, v.y, act), act_bwd1(d.z, v.z, act),
                                             act_bwd1(d.w, v.w, act));
                JP_F4W(dx)[i] = o;
                mx = fmaxf(fmaxf(mx, fmaxf(jp_fmag(o.x), jp_fmag(o.y))), fmaxf(jp_fmag(o.z), jp_fmag(o.w)));
            },
            [&](long i) {
                const float o = act_bwd1(dy[i], y[i], act);
                dx[i] = o;
                mx = fmaxf(mx, jp_fmag(o));
            });
    jp_block_amax_commit(mx, amax);
}

// activation backward + bias gradient in ONE pass over (N, C, HW): dx = dy * act'(y), dbias[c] += sum dx.  Replaces act_bwd followed
// by channel_sum (a second read of dx) for the convolutions that carry both a bias and an activation (Conv3x3 blocks, layers.py:147-167).
// grid (C, N * CH): block = one chunk of one (n, c) plane; fp32 short runs -> double, one float atomic per block (as channel_sum).
__global__ __launch_bounds__(TPB) void act_bwd_bias_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                                                           float* __restrict__ dbias, int C, int HW, int CH, int chunk, int act,
                                                           unsigned* __restrict__ amax, float* __restrict__ part) {
    __shared__ double sm[4];
    const int c = blockIdx.x;
    const int n = blockIdx.y / CH, ck = blockIdx.y - n * CH;
    const int beg = ck * chunk, end = min(HW, beg + chunk);
    const size_t base = ((size_t)n * C + c) * HW;
    double s = 0.0;
    float fs = 0.f, mx = 0.f;
    int run = 0;
    if (((HW | chunk) & 3) == 0) {
        const float4* d4 = reinterpret_cast<const float4*>(dy + base);
        const float4* y4 = reinterpret_cast<const float4*>(y + base);
        float4* o4 = reinterpret_cast<float4*>(dx + base);
        for (int i = (beg >> 2) + threadIdx.x; i < (end >> 2); i += TPB) {
            const float4 d = d4[i], v = y4[i];
            const float4 o = make_float4(act_bwd1(d.x, v.x, act), act_bwd1(d.y, v.y, act), act_bwd1(d.z, v.z, act), act_bwd1(d.w, v.w, act));
            o4[i] = o;
            mx = fmaxf(fmaxf(mx, fmaxf(jp_fmag(o.x), jp_fmag(o.y))), fmaxf(jp_fmag(o.z), jp_fmag(o.w)));
            fs += (o.x + o.y) + (o.z + o.w);
            if (++run == 8) { s += fs; fs = 0.f; run = 0; }
        }
    } else {
        for (int i = beg + threadIdx.x; i < end; i += TPB) {
            const float o = act_bwd1(dy[base + i], y[base + i], act);
            dx[base + i] = o;
            mx = fmaxf(mx, jp_fmag(o));
            fs += o;
            if (++run == 32) { s += fs; fs = 0.f; run = 0; }
        }
    }
    jp_block_amax_commit(mx, amax);
    s += fs;
    s = jp_block_sum_d(s, sm);
    if (threadIdx.x == 0) {
        if (part) part[(size_t)c * gridDim.y + blockIdx.y] = (float)s;      // fixed-order fold below: bit-reproducible
        else atomicAdd(&dbias[c], (float)s);
    }
}
// dbias[c] += part[c][0] + part[c][1] + ... in that order (one thread per channel)
__global__ void bias_fold_kernel(const float* __restrict__ part, float* __restrict__ dbias, int C, int S) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += part[(size_t)c * S + i];
    dbias[c] += s;
}

// out[n][c][hw] = a[n][c][hw] * s[n][0][hw]   (CrossViewTransformer.py:68) and its two adjoints
__global__ __launch_bounds__(TPB) void mul_bcast_c_kernel(const float* __restrict__ a, const float* __restrict__ s,
                                                          float* __restrict__ out, long total, int C, int HW) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int p = (int)(i % HW);
        const long n = i / ((long)C * HW);
        out[i] = a[i] * s[n * HW + p];
    }
}
__global__ __launch_bounds__(TPB) void mul_bcast_c_bwd_s_kernel(const float* __restrict__ dout,
                                                                const float* __restrict__ a, float* __restrict__ ds,
                                                                long total, int C, int HW) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int p = (int)(i % HW);
        const long n = i / HW;
        float g = 0.f;
        for (int c = 0; c < C; ++c) g += dout[(n * C + c) * HW + p] * a[(n * C + c) * HW + p];
        ds[i] = g;
    }
}

// ------------------------------------------------------------------ bilinear resize, align_corners=False
// (the sampling rule, bil_src / bil_sample, lives in bilinear.h: stream.hip resizes with the same bits)
__global__ __launch_bounds__(TPB) void bilinear_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           long total, int H, int W, int OH, int OW, float sy,
                                                           float sx) {
    for (long o = (long)blockIdx.x * TPB + threadIdx.x; o < total; o += (long)gridDim.x * TPB) {
        const int ox = (int)(o % OW);
        const long t = o / OW;
        const int oy = (int)(t % OH);
        const long nc = t / OH;
        y[o] = bil_sample(x + nc * H * W, oy, ox, H, W, sy, sx);
    }
}

// gather-form adjoint: input pixel i collects from every output whose 2x2 footprint touches it
__global__ __launch_bounds__(TPB) void bilinear_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                           long total, int H, int W, int OH, int OW, float sy,
                                                           float sx, int accumulate) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int ix = (int)(i % W);
        const long t = i / W;
        const int iy = (int)(t % H);
        const long nc = t / H;
        const float* dp = dy + nc * OH * OW;
        // outputs o with source coordinate in (i-1, i+1): o in ((i-0.5)/s-0.5, (i+1.5)/s-0.5), widened by 1
        int oy_lo = max(0, (int)floorf(((float)iy - 0.5f) / sy - 0.5f) - 1);
        int oy_hi = min(OH - 1, (int)ceilf(((float)iy + 1.5f) / sy - 0.5f) + 1);
        int ox_lo = max(0, (int)floorf(((float)ix - 0.5f) / sx - 0.5f) - 1);
        int ox_hi = min(OW - 1, (int)ceilf(((float)ix + 1.5f) / sx - 0.5f) + 1);
        if (iy == 0) oy_lo = 0;           // clamped sources (src < 0) all land on row/col 0
        if (ix == 0) ox_lo = 0;
        if (iy == H - 1) oy_hi = OH - 1;  // and sources beyond the last row on row H-1
        if (ix == W - 1) ox_hi = OW - 1;
        float g = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            int y0, y1;
            float wy;
            bil_src(oy, sy, H, y0, y1, wy);
            float cy = 0.f;
            if (y0 == iy) cy += 1.f - wy;
            if (y1 == iy) cy += wy;
            if (cy == 0.f) continue;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                int x0, x1;
                float wx;
                bil_src(ox, sx, W, x0, x1, wx);
                float cx = 0.f;
                if (x0 == ix) cx += 1.f - wx;
                if (x1 == ix) cx += wx;
                if (cx != 0.f) g += cy * cx * dp[oy * OW + ox];
            }
        }
        dx[i] = accumulate ? dx[i] + g : g;
    }
}

// F.interpolate(mode='area') with an integer factor f = H/OH = W/OW: mean of f x f blocks
__global__ __launch_bounds__(TPB) void area_down_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        long total, int H, int W, int OH, int OW, int f) {
    const float inv = 1.f / (float)(f * f);
    for (long o = (long)blockIdx.x * TPB + threadIdx.x; o < total; o += (long)gridDim.x * TPB) {
        const int ox = (int)(o % OW);
        const long t = o / OW;
        const int oy = (int)(t % OH);
        const long nc = t / OH;
        const float* xp = x + (nc * H + (long)oy * f) * W + (long)ox * f;
        float s = 0.f;
        for (int a = 0; a < f; ++a)
            for (int b = 0; b < f; ++b) s += xp[a * W + b];
        y[o] = s * inv;
    }
}

// torchgeometry-style warp_perspective (net.py:285-289,468-472): for every destination pixel, its
// normalised coordinate (linspace(-1,1)) is mapped by the 3x3 `src_norm_from_dst_norm` homography and the
// source is sampled bilinearly with zero padding (grid_sample, align_corners=False).  C == 1.
__global__ __launch_bounds__(TPB) void warp_perspective_kernel(const float* __restrict__ src,
                                                               const float* __restrict__ Hm, float* __restrict__ dst,
                                                               int h, int w, int OH, int OW) {
    const int b = blockIdx.y;
    const float* M = Hm + 9 * b;
    const float* sp = src + (size_t)b * h * w;
    for (int p = blockIdx.x * TPB + threadIdx.x; p < OH * OW; p += gridDim.x * TPB) {
        const int oy = p / OW, ox = p - oy * OW;
        const float gx = OW > 1 ? -1.f + 2.f * (float)ox / (float)(OW - 1) : -1.f;
        const float gy = OH > 1 ? -1.f + 2.f * (float)oy / (float)(OH - 1) : -1.f;
        const float X = M[0] * gx + M[1] * gy + M[2];
        const float Y = M[3] * gx + M[4] * gy + M[5];
        const float Z = M[6] * gx + M[7] * gy + M[8];
        const float sx = X / Z, sy = Y / Z;
        const float ix = ((sx + 1.f) * (float)w - 1.f) * 0.5f, iy = ((sy + 1.f) * (float)h - 1.f) * 0.5f;
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float tx = ix - fx, ty = iy - fy;
        float v = 0.f;
        if (ix == ix && iy == iy && fx > -2.f && fy > -2.f && fx < (float)w + 1.f && fy < (float)h + 1.f) {
            const bool xa = x0 >= 0 && x0 < w, xb = x0 + 1 >= 0 && x0 + 1 < w;
            const bool ya = y0 >= 0 && y0 < h, yb = y0 + 1 >= 0 && y0 + 1 < h;
            if (ya && xa) v += sp[y0 * w + x0] * (1.f - tx) * (1.f - ty);
            if (ya && xb) v += sp[y0 * w + x0 + 1] * tx * (1.f - ty);
            if (yb && xa) v += sp[(y0 + 1) * w + x0] * (1.f - tx) * ty;
            if (yb && xb) v += sp[(y0 + 1) * w + x0 + 1] * tx * ty;
        }
        dst[(size_t)b * OH * OW + p] = v;
    }
}

// nn.Softmax2d over C == 2 channels (eval-mode head of the BEV decoder, layout_model.py:194-199)
__global__ __launch_bounds__(TPB) void softmax_c2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         long total, int HW) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long n = i / HW;
        const int p = (int)(i - n * HW);
        const float a = x[(2 * n) * HW + p], b = x[(2 * n + 1) * HW + p];
        const float m = fmaxf(a, b);
        const float ea = __expf(a - m), eb = __expf(b - m);
        const float inv = 1.f / (ea + eb);
        y[(2 * n) * HW + p] = ea * inv;
        y[(2 * n + 1) * HW + p] = eb * inv;
    }
}

// depth = 1 / (min_disp + (max_disp - min_disp) * disp)   (layers.py:33-38)
__global__ __launch_bounds__(TPB) void disp_to_depth_kernel(const float* __restrict__ disp, float* __restrict__ depth,
                                                            long n, float min_disp, float max_disp) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB)
        depth[i] = 1.f / (min_disp + (max_disp - min_disp) * disp[i]);
}

// cv2.fillConvexPoly(img, pts, color, lineType=1) as the reference calls it (net.py:300-305,394-399): OpenCV 4.x
// drawing.cpp `FillConvexPoly` restated (third party, absent from the reference tree -> parity unpinned; the CPU
// restatement this kernel is tested against pixel-exactly is oracle/cv2_restated.py):
//   (1) every edge is drawn as a 4-connected Bresenham line (`Line(..., connectivity 1 -> 4)`, left-to-right,
//       clipped to the image by cv::clipLine);
//   (2) two-edge scan conversion in 16.16 fixed point, span of row y = [(xl + 0.5) >> 16, (xr + 0.5) >> 16].
// One workgroup-independent formulation: threads 0..npts-1 of block 0 walk one edge each; EVERY thread replays the
// (cheap, <= H iterations of integer arithmetic) scan-conversion state machine and emits only the rows dealt to it.
// mask (H x W bytes) must be zero on entry (the launcher clears it on the same stream).
__device__ inline bool cv_clip_line(long right, long bottom, long& x1, long& y1, long& x2, long& y2) {
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

constexpr int POLY_MAX = 8;
__global__ __launch_bounds__(TPB) void fill_convex_poly_kernel(const int* __restrict__ pts, int npts,
                                                               uint8_t* __restrict__ mask, int H, int W) {
    long vx[POLY_MAX], vy[POLY_MAX];
#pragma unroll
    for (int i = 0; i < POLY_MAX; ++i) {
        vx[i] = i < npts ? pts[2 * i] : 0;
        vy[i] = i < npts ? pts[2 * i + 1] : 0;
    }
    const int gt = blockIdx.x * TPB + threadIdx.x, nthreads = gridDim.x * TPB;
    if (gt < npts) {   // edge gt: v[gt-1] -> v[gt], LineIterator(connectivity 4, leftToRight)
        const int i0 = gt == 0 ? npts - 1 : gt - 1;
        long x1 = vx[i0], y1 = vy[i0], x2 = vx[gt], y2 = vy[gt];
        bool ok = true;
        if ((unsigned long)x1 >= (unsigned long)W || (unsigned long)x2 >= (unsigned long)W ||
            (unsigned long)y1 >= (unsigned long)H || (unsigned long)y2 >= (unsigned long)H)
            ok = cv_clip_line(W - 1, H - 1, x1, y1, x2, y2);
        if (ok) {
            long dx = x2 - x1, dy = y2 - y1, step_x = 1, step_y = 1;
            if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
            if (dy < 0) { dy = -dy; step_y = -1; }
            const bool vert = dy > dx;
            if (vert) { const long t = dx; dx = dy; dy = t; }
            long err = 0;
            const long plus = 2 * dx + 2 * dy, minus = -2 * dy, count = dx + dy + 1;
            long x = x1, y = y1;
            for (long k = 0; k < count; ++k) {
                mask[y * W + x] = 1;
                const bool m = err < 0;
                err += minus + (m ? plus : 0);
                // 4-connected: minor-axis step when the error went negative, else major-axis step
                if (vert) { if (m) x += step_x; else y += step_y; }
                else      { if (m) y += step_y; else x += step_x; }
            }
        }
    }
    if (npts < 3) return;
    long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    for (int i = 0; i < npts; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        ymax = vy[i] > ymax ? vy[i] : ymax;
        xmax = vx[i] > xmax ? vx[i] : xmax;
        xmin = vx[i] < xmin ? vx[i] : xmin;
    }
    if (xmax < 0 || ymax < 0 || xmin >= W || ymin >= H) return;
    if (ymax > H - 1) ymax = H - 1;
    int e_idx[2] = {imin, imin};
    const int e_di[2] = {1, npts - 1};
    long e_x[2] = {-65536, -65536}, e_dx[2] = {0, 0}, e_ye[2] = {ymin, ymin};
    int edges = npts;
    long y = ymin;
    do {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (y >= e_ye[i]) {
                int idx0 = e_idx[i], idx = idx0 + e_di[i];
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    long ty = 0, xs = 0, xe = 0;
#pragma unroll
                    for (int q = 0; q < POLY_MAX; ++q) {      // register-array select (no scratch indexing)
                        if (q == idx) { ty = vy[q]; xe = vx[q]; }
                        if (q == idx0) xs = vx[q];
                    }
                    if (ty > y) {
                        xs <<= 16;
                        xe <<= 16;
                        e_ye[i] = ty;
                        e_dx[i] = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));   // C division truncates like OpenCV's
                        e_x[i] = xs;
                        e_idx[i] = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += e_di[i];
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0 && (int)((y - (ymin < 0 ? 0 : ymin)) % nthreads) == gt) {
            const int l = e_x[0] > e_x[1] ? 1 : 0;
            long xx1 = (e_x[l] + 32768) >> 16, xx2 = (e_x[1 - l] + 32768) >> 16;
            if (xx2 >= 0 && xx1 < W) {
                if (xx1 < 0) xx1 = 0;
                if (xx2 >= W) xx2 = W - 1;
                for (long x = xx1; x <= xx2; ++x) mask[y * W + x] = 1;
            }
        }
        e_x[0] += e_dx[0];
        e_x[1] += e_dx[1];
    } while (++y <= ymax);
}

// CGT scale label assembly (net.py:291-309 static / :394-401 dynamic / :474-475 both):
//   mode 0: out = zwarp * laywarp                                   (Argo_both)
//   mode 1: out = zwarp * uint8(laywarp) * polymask                 (static; laywarp == NULL -> dynamic)
// `.type_as(uint8)` keeps the pixels whose bilinearly warped {0,1} layout reaches 1.0; the interpolation weights
// sum to 1 only up to fp32 rounding (platform-dependent in the reference itself), so "reaches 1" is taken with a
// 1e-6 guard band.  polymask = the H x W byte mask of jp_fill_convex_poly (shared by the whole batch, like the
// reference's batch-item-0 polygon).
__global__ __launch_bounds__(TPB) void scale_label_kernel(const float* __restrict__ zw, const float* __restrict__ lw,
                                                          const uint8_t* __restrict__ polymask, float* __restrict__ out,
                                                          long total, long HW, int mode) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        float m = lw ? lw[i] : 1.f;
        if (mode == 1) {
            m = (lw == nullptr || m >= 0.999999f) ? 1.f : 0.f;
            if (!polymask[i % HW]) m = 0.f;
        }
        out[i] = zw[i] * m;
    }
}

}  // namespace

#define JP_ST hipStream_t st = (hipStream_t)stream

extern "C" int jp_maxpool_fwd(const float* x, float* y, uint8_t* idx, int NC, int H, int W, int k, int s, int p,
                              void* stream) {
    JP_CHECK_ARG(x && y && idx && NC > 0 && NC <= 65535 && k >= 1 && k <= 7 && s >= 1 && s <= 2, "maxpool_fwd: bad args");
    JP_ST;
    const int OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
    const dim3 gt(jp_cdiv(OW, MP_TW), jp_cdiv(OH, MPF_TH), NC);
    if (pool5_rows_ok(k, s, p, W)) {   // CRP maps: row-streaming kernel (wave shuffles, no LDS tile)
        pool5_rows(true, x, y, idx, nullptr, nullptr, NC, H, W, st);
        JP_LAUNCH_CHECK();
    }
    if (k == 5 && s == 1) {
        hipLaunchKernelGGL((maxpool_fwd_t_kernel<5, 1>), gt, dim3(TPB), 0, st, x, y, idx, H, W, OH, OW, p);
        JP_LAUNCH_CHECK();
    }
    if (k == 3 && s == 2) {
        hipLaunchKernelGGL((maxpool_fwd_t_kernel<3, 2>), gt, dim3(TPB), 0, st, x, y, idx, H, W, OH, OW, p);
        JP_LAUNCH_CHECK();
    }
    if (k == 2 && s == 2) {
        hipLaunchKernelGGL((maxpool_fwd_t_kernel<2, 2>), gt, dim3(TPB), 0, st, x, y, idx, H, W, OH, OW, p);
        JP_LAUNCH_CHECK();
    }
    const int pw = (MP_TW - 1) * s + k, ph = (MP_TH - 1) * s + k;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(jp_cdiv(OW, MP_TW), jp_cdiv(OH, MP_TH), NC), dim3(TPB),
                       sizeof(float) * pw * ph, st, x, y, idx, H, W, OH, OW, k, s, p);
    JP_LAUNCH_CHECK();
}

// dx = (addend ? addend : 0) + scatter of dy through the saved argmax; `addend` (may be NULL, may not alias dx) lets a
// residual branch's gradient be folded in without a separate accumulation pass (CRP chains, layers.py:193-198)
extern "C" int jp_amax_into(const float* x, long n, float* out, void* stream);
// amax_dx: optional magnitude slot (see the header) that receives max |dx| -- folded in by the 5x5 row kernel itself, by a reduction
// pass behind the other kernels
extern "C" int jp_maxpool_bwd(const float* dy, const uint8_t* idx, float* dx, const float* addend, int NC, int H,
                              int W, int k, int s, int p, float* amax_dx, void* stream) {
    JP_CHECK_ARG(dy && dx && idx && NC > 0 && NC <= 65535 && k >= 1 && k <= 7 && s >= 1 && s <= 2, "maxpool_bwd: bad args");
    JP_ST;
    const int OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
    if (pool5_rows_ok(k, s, p, W)) {
        pool5_rows(false, dy, dx, nullptr, idx, addend, NC, H, W, st, reinterpret_cast<unsigned*>(amax_dx));
        JP_LAUNCH_CHECK();
    }
    if (k == 5 && s == 1) {
        hipLaunchKernelGGL((maxpool_bwd_s1_kernel<5>), dim3(jp_cdiv(W, MP_TW), jp_cdiv(H, MPF_TH), NC), dim3(TPB), 0, st,
                           dy, idx, dx, addend, H, W, OH, OW, p);
    } else if (k == 3 && s == 2 && p == 1 && H == 2 * OH && W == 2 * OW && OW % 2 == 0) {
        const int RB = OH >= 128 ? 32 : 8, bands = jp_cdiv(OH, RB);
        const long units = (long)NC * bands * (OW / 2);
        hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3((unsigned)jp_cdiv(units, (long)TPB)), dim3(TPB), 0, st, dy, idx, dx, addend,
                           units, OH, OW, RB, bands);
    } else {
        // outputs that can cover a 64x8 input tile
        const int pw = (MP_TW + k - 2) / s + 2, ph = (MP_TH + k - 2) / s + 2;
        hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(jp_cdiv(W, MP_TW), jp_cdiv(H, MP_TH), NC), dim3(TPB),
                           2 * sizeof(float) * pw * ph, st, dy, idx, dx, addend, H, W, OH, OW, k, s, p, pw, ph);
    }
    if (amax_dx) return jp_amax_into(dx, (long)NC * H * W, amax_dx, stream);
    JP_LAUNCH_CHECK();
}

// y[n][dc0 + c] = nearest-2x(x[n][c]) written into a channel slice of a (N, dstC, 2H, 2W) tensor
extern "C" int jp_upsample2x_fwd(const float* x, float* y, int N, int C, int H, int W, int dstC, int dc0,
                                 void* stream) {
    JP_CHECK_ARG(x && y && N > 0 && C > 0 && dc0 + C <= dstC, "upsample2x_fwd: bad args");
    JP_ST;
    const long total = (long)N * C * H * W * 4;
    if (W % 4 == 0 && total / 16 < (1L << 31)) {
        hipLaunchKernelGGL(upsample2x_fwd_v4_kernel, dim3(blocks_for(total / 16)), dim3(TPB), 0, st, x, y,
                           (unsigned)(total / 16), C, H, W / 4, dstC, dc0);
        JP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, x, y, total, C, H, W, dstC, dc0);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_upsample2x_bwd(const float* dy, float* dx, int N, int C, int H, int W, int Ctot, int c0,
                                 int accumulate, void* stream) {
    JP_CHECK_ARG(dy && dx && N > 0 && C > 0 && c0 + C <= Ctot, "upsample2x_bwd: bad args");
    JP_ST;
    const long total = (long)N * C * H * W;
    if (W % 2 == 0 && total < (1L << 31)) {
        hipLaunchKernelGGL(upsample2x_bwd_v2_kernel, dim3(blocks_for(total / 2)), dim3(TPB), 0, st, dy, dx,
                           (unsigned)(total / 2), C, H, W / 2, Ctot, c0, accumulate);
        JP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, dy, dx, total, C, H, W, Ctot,
                       c0, accumulate);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_copy_channels(const float* src, float* dst, int N, int C, int HW, int srcC, int sc0, int dstC,
                                int dc0, int accumulate, void* stream) {
    JP_CHECK_ARG(src && dst && N > 0 && C > 0 && sc0 + C <= srcC && dc0 + C <= dstC, "copy_channels: bad args");
    JP_ST;
    const long total = (long)N * C * HW;
    if (HW % 4 == 0 && total < (1L << 32)) {
        hipLaunchKernelGGL(copy_channels_v4_kernel, dim3(blocks_for(total / 4)), dim3(TPB), 0, st, src, dst,
                           (unsigned)(total / 4), C, HW / 4, srcC, sc0, dstC, dc0, accumulate);
        JP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(copy_channels_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, src, dst, total, C, HW, srcC,
                       sc0, dstC, dc0, accumulate);
    JP_LAUNCH_CHECK();
}

// amax_out: optional magnitude slot (see the header) that receives max |out|
extern "C" int jp_sum_n(const float* a0, const float* a1, const float* a2, const float* a3, const float* a4, float* out,
                        long n, float* amax_out, void* stream) {
    JP_CHECK_ARG(a0 && a1 && out && n > 0 && !(a3 && !a2) && !(a4 && !a3), "sum_n: bad args");
    JP_ST;
    hipLaunchKernelGGL(sum_n_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, a0, a1, a2, a3, a4, out, n,
                       reinterpret_cast<unsigned*>(amax_out));
    JP_LAUNCH_CHECK();
}

extern "C" int jp_axpby(const float* a, const float* b, float* out, long n, float alpha, float beta, void* stream) {
    JP_CHECK_ARG(a && out && n > 0, "axpby: bad args");
    JP_ST;
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, a, b, out, n, alpha, beta);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_mul(const float* a, const float* b, float* out, long n, float scale, void* stream) {
    JP_CHECK_ARG(a && b && out && n > 0, "mul: bad args");
    JP_ST;
    hipLaunchKernelGGL(mul_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, a, b, out, n, scale);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_affine(const float* a, float* out, long n, float scale, float shift, void* stream) {
    JP_CHECK_ARG(a && out && n > 0, "affine: bad args");
    JP_ST;
    hipLaunchKernelGGL(affine_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, a, out, n, scale, shift);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_act_fwd(const float* x, float* y, long n, int act, void* stream) {
    JP_CHECK_ARG(x && y && n > 0, "act_fwd: bad args");
    JP_ST;
    hipLaunchKernelGGL(act_fwd_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, x, y, n, act);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_act_bwd(const float* dy, const float* y, float* dx, long n, int act, float* amax_dx, void* stream) {
    JP_CHECK_ARG(dy && y && dx && n > 0, "act_bwd: bad args");
    JP_ST;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(blocks_for((n + 3) / 4)), dim3(TPB), 0, st, dy, y, dx, n, act, reinterpret_cast<unsigned*>(amax_dx));
    JP_LAUNCH_CHECK();
}

// dx = dy * act'(y) and dbias[c] += sum over (n, hw) of dx, one pass (dbias is accumulated into: zero it for a fresh gradient).
// bias_ws: optional scratch of jp_act_bwd_bias_ws_floats(N, C, HW) floats -- the per-workgroup partial sums are then folded in a fixed
// order (bit-reproducible bias gradients); NULL: they meet in float atomics (run-dependent last bits)
static void act_bias_chunks(int N, int C, int HW, int* CH, int* chunk) {
    int ch = std::max(1, 2048 / std::max(1, N * C));
    ch = std::min(ch, std::max(1, HW / 2048));
    int ck = (HW + ch - 1) / ch;
    ck = (ck + 3) & ~3;                             // chunks start on 16-byte boundaries when HW allows vector accesses
    *chunk = ck;
    *CH = (HW + ck - 1) / ck;
}
extern "C" long jp_act_bwd_bias_ws_floats(int N, int C, int HW) {
    int CH, chunk;
    act_bias_chunks(N, C, HW, &CH, &chunk);
    return (long)C * N * CH;
}
extern "C" int jp_act_bwd_bias(const float* dy, const float* y, float* dx, float* dbias, int N, int C, int HW, int act,
                               float* amax_dx, float* bias_ws, void* stream) {
    JP_CHECK_ARG(dy && y && dx && dbias && N > 0 && C > 0 && HW > 0 && C <= 65535, "act_bwd_bias: bad args");
    JP_ST;
    int CH, chunk;
    act_bias_chunks(N, C, HW, &CH, &chunk);
    JP_CHECK_ARG((long)N * CH <= 65535, "act_bwd_bias: too many chunks");
    hipLaunchKernelGGL(act_bwd_bias_kernel, dim3(C, N * CH), dim3(TPB), 0, st, dy, y, dx, dbias, C, HW, CH, chunk, act,
                       reinterpret_cast<unsigned*>(amax_dx), bias_ws);
    if (bias_ws) hipLaunchKernelGGL(bias_fold_kernel, dim3(jp_cdiv(C, 64)), dim3(64), 0, st, bias_ws, dbias, C, N * CH);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_mul_bcast_c(const float* a, const float* s, float* out, int N, int C, int HW, void* stream) {
    JP_CHECK_ARG(a && s && out && N > 0, "mul_bcast_c: bad args");
    JP_ST;
    const long total = (long)N * C * HW;
    hipLaunchKernelGGL(mul_bcast_c_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, a, s, out, total, C, HW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_mul_bcast_c_bwd_s(const float* dout, const float* a, float* ds, int N, int C, int HW,
                                    void* stream) {
    JP_CHECK_ARG(dout && a && ds && N > 0, "mul_bcast_c_bwd_s: bad args");
    JP_ST;
    const long total = (long)N * HW;
    hipLaunchKernelGGL(mul_bcast_c_bwd_s_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, dout, a, ds, total, C, HW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_bilinear_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, void* stream) {
    JP_CHECK_ARG(x && y && NC > 0 && OH > 0 && OW > 0, "bilinear_fwd: bad args");
    JP_ST;
    const long total = (long)NC * OH * OW;
    hipLaunchKernelGGL(bilinear_fwd_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, x, y, total, H, W, OH, OW,
                       (float)H / (float)OH, (float)W / (float)OW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_bilinear_bwd(const float* dy, float* dx, int NC, int H, int W, int OH, int OW, int accumulate,
                               void* stream) {
    JP_CHECK_ARG(dy && dx && NC > 0, "bilinear_bwd: bad args");
    JP_ST;
    const long total = (long)NC * H * W;
    hipLaunchKernelGGL(bilinear_bwd_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, dy, dx, total, H, W, OH, OW,
                       (float)H / (float)OH, (float)W / (float)OW, accumulate);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_area_downsample(const float* x, float* y, int NC, int H, int W, int f, void* stream) {
    JP_CHECK_ARG(x && y && NC > 0 && f >= 1 && H % f == 0 && W % f == 0, "area_downsample: bad args");
    JP_ST;
    const long total = (long)NC * (H / f) * (W / f);
    hipLaunchKernelGGL(area_down_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, x, y, total, H, W, H / f, W / f, f);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_warp_perspective(const float* src, const float* Hm, float* dst, int B, int h, int w, int OH, int OW,
                                   void* stream) {
    JP_CHECK_ARG(src && Hm && dst && B > 0, "warp_perspective: bad args");
    JP_ST;
    hipLaunchKernelGGL(warp_perspective_kernel, dim3(std::min(jp_cdiv((long)OH * OW, TPB), 4096), B), dim3(TPB), 0, st,
                       src, Hm, dst, h, w, OH, OW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_softmax_c2(const float* x, float* y, int N, int HW, void* stream) {
    JP_CHECK_ARG(x && y && N > 0 && HW > 0, "softmax_c2: bad args");
    JP_ST;
    const long total = (long)N * HW;
    hipLaunchKernelGGL(softmax_c2_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, x, y, total, HW);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_disp_to_depth(const float* disp, float* depth, long n, float min_depth, float max_depth,
                                void* stream) {
    JP_CHECK_ARG(disp && depth && n > 0, "disp_to_depth: bad args");
    JP_ST;
    hipLaunchKernelGGL(disp_to_depth_kernel, dim3(blocks_for(n)), dim3(TPB), 0, st, disp, depth, n, 1.f / max_depth,
                       1.f / min_depth);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_fill_convex_poly(const int* pts, int npts, uint8_t* mask, int H, int W, void* stream) {
    JP_CHECK_ARG(pts && mask && npts >= 1 && npts <= POLY_MAX && H > 0 && W > 0, "fill_convex_poly: bad args");
    JP_ST;
    JP_HIP(hipMemsetAsync(mask, 0, (size_t)H * W, st));
    hipLaunchKernelGGL(fill_convex_poly_kernel, dim3(8), dim3(TPB), 0, st, pts, npts, mask, H, W);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_scale_label_assemble(const float* zwarp, const float* laywarp, const uint8_t* polymask, float* out,
                                       int B, int H, int W, int mode, void* stream) {
    JP_CHECK_ARG(zwarp && out && B > 0 && (mode == 0 || polymask), "scale_label_assemble: bad args");
    JP_ST;
    const long total = (long)B * H * W;
    hipLaunchKernelGGL(scale_label_kernel, dim3(blocks_for(total)), dim3(TPB), 0, st, zwarp, laywarp, polymask, out,
                       total, (long)H * W, mode);
    JP_LAUNCH_CHECK();
}
