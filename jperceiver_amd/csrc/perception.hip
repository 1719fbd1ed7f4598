// Post-processing of the video perception API (jperceiver_amd/apis/perception.py) -- what scripts/eval_kitti_video.py does in
// host numpy on copied-back tensors, as streaming kernels on the device:
//   jp_disp_resize_depth : disp_to_depth's scaled disparity -> cv2.resize(INTER_LINEAR) -> 1/x, one pass      (:121-133)
//   jp_quantiles         : exact order statistics of every row (np.percentile / the minimum of plt.imsave's Normalize)
//   jp_colorize_u8       : matplotlib Normalize(vmin, vmax) + a 256-entry colormap                              (:134-136)
//   jp_layout_classes_u8 : argmax of the road and the car head -> class map -> palette                          (:157-161,195-218)
// All of them are bandwidth-bound: 16-byte loads and whole-dword stores where the row length and the pointers allow it, a
// scalar path otherwise; grids of at most 2048 workgroups of 256 threads (4 waves of 64) that stride over the rest.
#include "jp_common.h"
#include <algorithm>
#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_BLOCKS = 2048;      // 256 CUs x 8 resident workgroups

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
inline int grid_for(long work) { return (int)std::max<long>(1, std::min<long>((work + TPB - 1) / TPB, MAX_BLOCKS)); }

// ------------------------------------------------------------------ (a) scaled disparity -> bilinear resize -> depth
// the sampling rule of jp_bilinear_fwd (pointwise.hip:bil_src): PyTorch's area_pixel_compute_source_index, align_corners=False
__device__ __forceinline__ void bil_src(int o, float scale, int in, int& i0, int& i1, float& w1) {
    float src = ((float)o + 0.5f) * scale - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    w1 = src - (float)i0;
}

__device__ __forceinline__ float drd_sample(const float* __restrict__ r0, const float* __restrict__ r1, int ox, float sx, int w,
                                            float wy, float scale, float shift) {
    int x0, x1;
    float wx;
    bil_src(ox, sx, w, x0, x1, wx);
    const float a = r0[x0] * scale + shift, b = r0[x1] * scale + shift, c = r1[x0] * scale + shift, d = r1[x1] * scale + shift;
    return (1.f - wy) * ((1.f - wx) * a + wx * b) + wy * ((1.f - wx) * c + wx * d);
}

// VEC: every thread writes 4 consecutive pixels of one output row with one 16-byte store per output (OW % 4 == 0, aligned bases)
template <bool VEC>
__global__ __launch_bounds__(TPB) void disp_resize_depth_kernel(const float* __restrict__ disp, float* __restrict__ depth,
                                                                float* __restrict__ sdisp, long total, int h, int w, int OH,
                                                                int OW, float sy, float sx, float scale, float shift) {
    constexpr int V = VEC ? 4 : 1;
    const int OWV = OW / V;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int oxv = (int)(i % OWV);
        const long t = i / OWV;
        const int oy = (int)(t % OH);
        const long b = t / OH;
        int y0, y1;
        float wy;
        bil_src(oy, sy, h, y0, y1, wy);
        const float* r0 = disp + (b * h + y0) * (long)w;
        const float* r1 = disp + (b * h + y1) * (long)w;
        const long o = (b * OH + oy) * (long)OW + (long)oxv * V;
        if constexpr (VEC) {
            float4 s;
            s.x = drd_sample(r0, r1, oxv * 4 + 0, sx, w, wy, scale, shift);
            s.y = drd_sample(r0, r1, oxv * 4 + 1, sx, w, wy, scale, shift);
            s.z = drd_sample(r0, r1, oxv * 4 + 2, sx, w, wy, scale, shift);
            s.w = drd_sample(r0, r1, oxv * 4 + 3, sx, w, wy, scale, shift);
            *reinterpret_cast<float4*>(depth + o) = make_float4(1.f / s.x, 1.f / s.y, 1.f / s.z, 1.f / s.w);
            if (sdisp) *reinterpret_cast<float4*>(sdisp + o) = s;
        } else {
            const float s = drd_sample(r0, r1, oxv, sx, w, wy, scale, shift);
            depth[o] = 1.f / s;
            if (sdisp) sdisp[o] = s;
        }
    }
}

// ------------------------------------------------------------------ (b) exact order statistics by radix selection
// Order-preserving unsigned key of a float in np.sort's order: negatives below positives, -0.0 next to +0.0 (either is an accepted
// answer where they tie), +-Inf as values, every NaN (of either sign) last.
__device__ __forceinline__ unsigned q_key(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float q_val(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);      // 0xffffffff -> 0x7fffffff, a NaN
}

constexpr int Q_MAXQ = 4, Q_T = 2 * Q_MAXQ;         // targets of a row: the two neighbouring order statistics of every q
constexpr int Q_BINS = 256, Q_PASSES = 4;           // 8 key bits per pass, most significant first
constexpr int Q_MAXROWS = 64;

// per-row selection state between the passes (in ws, behind the histograms)
struct QState {
    unsigned prefix[Q_T];       // key bits fixed so far, per target
    unsigned krem[Q_T];         // rank of the target among the elements that share its prefix
    unsigned lead[Q_T];         // index into uprefix of the target's prefix
    unsigned uprefix[Q_T];      // the distinct prefixes: one histogram each
    unsigned nuniq;
    unsigned pad[31];           // 256 bytes
};
struct QRanks { unsigned k[Q_T]; };

// h[digit] += 1 for the lanes with m set.  Depth-like data puts a whole wave into ONE bin in the leading passes (same sign and
// exponent), which a per-lane LDS atomic serialises 64-fold: a wave that agrees on the bin adds its count once.
// Must be reached by all 64 lanes.
__device__ __forceinline__ void q_hist_add(unsigned* h, unsigned digit, bool m) {
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

// hist[row][u][digit] += #{ elements of the row whose leading 8*pass key bits equal uprefix[u] and whose next 8 bits are digit }
template <bool VEC>
__global__ __launch_bounds__(TPB) void q_hist_kernel(const float* __restrict__ x, int n, const QState* __restrict__ state,
                                                     unsigned* __restrict__ hist, int pass) {
    __shared__ unsigned sh[Q_T * Q_BINS];
    __shared__ unsigned up[Q_T];
    const int row = blockIdx.y;
    const int nu = pass == 0 ? 1 : (int)state[row].nuniq;
    if (threadIdx.x < Q_T) up[threadIdx.x] = pass == 0 ? 0u : state[row].uprefix[threadIdx.x];
    for (int i = threadIdx.x; i < nu * Q_BINS; i += TPB) sh[i] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const float* xr = x + (size_t)row * n;
    constexpr int V = VEC ? 4 : 1;
    const int nv = n / V;                              // VEC: n % 4 == 0
    for (int base = blockIdx.x * TPB; base < nv; base += gridDim.x * TPB) {      // wave-uniform trip count
        const int i = base + threadIdx.x;
        const bool ok = i < nv;
        float v[V];
        if constexpr (VEC) {
            const float4 f = ok ? reinterpret_cast<const float4*>(xr)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
            v[0] = ok ? xr[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const unsigned key = q_key(v[j]);
            const unsigned hi = pass == 0 ? 0u : key >> (shift + 8);
            const unsigned digit = (key >> shift) & 255u;
            for (int u = 0; u < nu; ++u) q_hist_add(sh + u * Q_BINS, digit, ok && hi == up[u]);
        }
    }
    __syncthreads();
    unsigned* hr = hist + (size_t)row * Q_T * Q_BINS;
    for (int i = threadIdx.x; i < nu * Q_BINS; i += TPB)
        if (sh[i]) atomicAdd(&hr[i], sh[i]);           // integer sums: the same total for every arrival order
}

// one workgroup per row: every target walks its histogram to the bin that holds its rank, which fixes 8 more key bits
__global__ __launch_bounds__(Q_BINS) void q_pick_kernel(QState* __restrict__ state, const unsigned* __restrict__ hist, int pass,
                                                        int nt, QRanks ranks, float* __restrict__ out) {
    __shared__ unsigned sc[Q_BINS];
    __shared__ unsigned np[Q_T], nk[Q_T];
    const int row = blockIdx.x, tid = threadIdx.x;
    QState& st = state[row];
    const unsigned* hr = hist + (size_t)row * Q_T * Q_BINS;
    for (int t = 0; t < nt; ++t) {
        const unsigned u = pass == 0 ? 0u : st.lead[t];
        const unsigned kr = pass == 0 ? ranks.k[t] : st.krem[t];
        const unsigned pf = pass == 0 ? 0u : st.prefix[t];
        const unsigned h = hr[u * Q_BINS + tid];
        sc[tid] = h;
        __syncthreads();
        for (int o = 1; o < Q_BINS; o <<= 1) {          // inclusive scan of the 256 bins
            const unsigned add = tid >= o ? sc[tid - o] : 0u;
            __syncthreads();
            sc[tid] += add;
            __syncthreads();
        }
        const unsigned incl = sc[tid], excl = incl - h;
        if (h != 0 && excl <= kr && kr < incl) {        // exactly one bin: the counts of a prefix sum to more than its rank
            np[t] = (pf << 8) | (unsigned)tid;
            nk[t] = kr - excl;
        }
        __syncthreads();
    }
    if (tid == 0) {
        unsigned nuq = 0;
        for (int t = 0; t < nt; ++t) {
            st.prefix[t] = np[t];
            st.krem[t] = nk[t];
            unsigned u = 0;
            while (u < nuq && st.uprefix[u] != np[t]) ++u;
            if (u == nuq) st.uprefix[nuq++] = np[t];
            st.lead[t] = u;
            if (pass == Q_PASSES - 1) out[(size_t)row * nt + t] = q_val(np[t]);
        }
        st.nuniq = nuq;
    }
}

// ------------------------------------------------------------------ (c) Normalize + 256-entry colormap
// four RGB triples (r | g << 8 | b << 16) -> the 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 as three dwords
__device__ __forceinline__ void pack_rgb4(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* __restrict__ dst) {
    dst[0] = c0 | (c1 << 24);
    dst[1] = (c1 >> 8) | (c2 << 16);
    dst[2] = (c2 >> 16) | (c3 << 8);
}

// fp32, in this order and unfused: (x - vmin) * (256 / (vmax - vmin)), floor, clamp to 0..255; 0 where vmax <= vmin.
// The clamp is applied to the floored float (the same result, and the conversion never sees a value outside int's range);
// a NaN lands on 0.
__device__ __forceinline__ int col_index(float x, float vmin, float s, bool flat) {
    const float v = floorf(__fmul_rn(__fsub_rn(x, vmin), s));
    return flat ? 0 : (int)fminf(fmaxf(v, 0.f), 255.f);
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void colorize_kernel(const float* __restrict__ x, int n, const float* __restrict__ vmm,
                                                       const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
    __shared__ unsigned pal[256];
    const int row = blockIdx.y;
    pal[threadIdx.x] = (unsigned)lut[3 * threadIdx.x] | ((unsigned)lut[3 * threadIdx.x + 1] << 8) |
                       ((unsigned)lut[3 * threadIdx.x + 2] << 16);
    __syncthreads();
    const float vmin = vmm[2 * row], vmax = vmm[2 * row + 1];
    const bool flat = !(vmax > vmin);
    const float s = __fdiv_rn(256.0f, __fsub_rn(vmax, vmin));
    const float* xr = x + (size_t)row * n;
    uint8_t* orow = out + (size_t)row * n * 3;
    if constexpr (VEC) {
        const int n4 = n / 4;
        for (int i = blockIdx.x * TPB + threadIdx.x; i < n4; i += gridDim.x * TPB) {
            const float4 f = reinterpret_cast<const float4*>(xr)[i];
            pack_rgb4(pal[col_index(f.x, vmin, s, flat)], pal[col_index(f.y, vmin, s, flat)], pal[col_index(f.z, vmin, s, flat)],
                      pal[col_index(f.w, vmin, s, flat)], reinterpret_cast<unsigned*>(orow) + 3 * (size_t)i);
        }
    } else {
        for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
            const unsigned c = pal[col_index(xr[i], vmin, s, flat)];
            orow[3 * (size_t)i] = (uint8_t)c;
            orow[3 * (size_t)i + 1] = (uint8_t)(c >> 8);
            orow[3 * (size_t)i + 2] = (uint8_t)(c >> 16);
        }
    }
}

// ------------------------------------------------------------------ (d) two 2-channel heads -> class map (+ palette)
// np.argmax's first maximum: class 1 / 2 only where channel 1 is STRICTLY greater; the car head overrides the road head
__device__ __forceinline__ unsigned lay_class(float r0, float r1, float c0, float c1) {
    return c1 > c0 ? 2u : (r1 > r0 ? 1u : 0u);
}
__device__ __forceinline__ unsigned lay_rgb(unsigned c) {        // 0 -> (0,0,0), 1 -> (255,255,255), 2 -> (0,0,255)
    return c == 1u ? 0x00ffffffu : (c == 2u ? 0x00ff0000u : 0u);
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void layout_classes_kernel(const float* __restrict__ road, const float* __restrict__ car,
                                                             uint8_t* __restrict__ cls, uint8_t* __restrict__ rgb, int HW) {
    const int b = blockIdx.y;
    const float* r0 = road + (size_t)b * 2 * HW;
    const float* r1 = r0 + HW;
    const float* c0 = car ? car + (size_t)b * 2 * HW : nullptr;
    const float* c1 = car ? c0 + HW : nullptr;
    uint8_t* cb = cls + (size_t)b * HW;
    uint8_t* pb = rgb ? rgb + (size_t)b * HW * 3 : nullptr;
    if constexpr (VEC) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = blockIdx.x * TPB + threadIdx.x; i < HW / 4; i += gridDim.x * TPB) {
            const float4 a0 = reinterpret_cast<const float4*>(r0)[i], a1 = reinterpret_cast<const float4*>(r1)[i];
            const float4 b0 = car ? reinterpret_cast<const float4*>(c0)[i] : z, b1 = car ? reinterpret_cast<const float4*>(c1)[i] : z;
            const unsigned k0 = lay_class(a0.x, a1.x, b0.x, b1.x), k1 = lay_class(a0.y, a1.y, b0.y, b1.y),
                           k2 = lay_class(a0.z, a1.z, b0.z, b1.z), k3 = lay_class(a0.w, a1.w, b0.w, b1.w);
            reinterpret_cast<unsigned*>(cb)[i] = k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
            if (pb) pack_rgb4(lay_rgb(k0), lay_rgb(k1), lay_rgb(k2), lay_rgb(k3), reinterpret_cast<unsigned*>(pb) + 3 * (size_t)i);
        }
    } else {
        for (int i = blockIdx.x * TPB + threadIdx.x; i < HW; i += gridDim.x * TPB) {
            const unsigned k = lay_class(r0[i], r1[i], car ? c0[i] : 0.f, car ? c1[i] : 0.f);
            cb[i] = (uint8_t)k;
            if (pb) {
                const unsigned c = lay_rgb(k);
                pb[3 * (size_t)i] = (uint8_t)c;
                pb[3 * (size_t)i + 1] = (uint8_t)(c >> 8);
                pb[3 * (size_t)i + 2] = (uint8_t)(c >> 16);
            }
        }
    }
}
}  // namespace

#define JP_ST hipStream_t st = (hipStream_t)stream

// disp (B,1,h,w) in [0,1] -> depth_out (B,1,OH,OW) = 1 / resize(1/max_depth + (1/min_depth - 1/max_depth) * disp);
// disp_out (nullable): the resized scaled disparity itself
extern "C" int jp_disp_resize_depth(const float* disp, float* depth_out, float* disp_out, int B, int h, int w, int OH, int OW,
                                    double min_depth, double max_depth, void* stream) {
    JP_CHECK_ARG(disp && depth_out, "disp_resize_depth: null pointer");
    JP_CHECK_ARG(B > 0 && h > 0 && w > 0 && OH > 0 && OW > 0, "disp_resize_depth: non-positive size");
    JP_CHECK_ARG(min_depth > 0.0 && max_depth > min_depth, "disp_resize_depth: need 0 < min_depth < max_depth");
    JP_ST;
    const float scale = (float)(1.0 / min_depth - 1.0 / max_depth), shift = (float)(1.0 / max_depth);
    const float sy = (float)h / (float)OH, sx = (float)w / (float)OW;
    const bool vec = OW % 4 == 0 && al16(depth_out) && (!disp_out || al16(disp_out));
    const long total = (long)B * OH * (vec ? OW / 4 : OW);
    if (vec)
        hipLaunchKernelGGL(disp_resize_depth_kernel<true>, dim3(grid_for(total)), dim3(TPB), 0, st, disp, depth_out, disp_out, total,
                           h, w, OH, OW, sy, sx, scale, shift);
    else
        hipLaunchKernelGGL(disp_resize_depth_kernel<false>, dim3(grid_for(total)), dim3(TPB), 0, st, disp, depth_out, disp_out, total,
                           h, w, OH, OW, sy, sx, scale, shift);
    JP_LAUNCH_CHECK();
}

// bytes of caller scratch for jp_quantiles on `rows` rows (need not be initialised)
extern "C" long jp_quantiles_ws_bytes(int rows) {
    JP_CHECK_ARG(rows > 0 && rows <= Q_MAXROWS, "quantiles_ws_bytes: rows must be 1..64");
    return (long)rows * ((long)Q_PASSES * Q_T * Q_BINS * sizeof(unsigned) + sizeof(QState));
}

// x (rows, n); q: HOST array of nq <= 4 values in [0,1]; out (rows, nq, 2): the order statistics k = floor(q (n-1)) and
// min(k+1, n-1) of every row -- the two values numpy's `linear` quantile interpolates between.
extern "C" int jp_quantiles(const float* x, int rows, int n, const float* q, int nq, float* out, void* ws, void* stream) {
    JP_CHECK_ARG(x && q && out && ws, "quantiles: null pointer");
    JP_CHECK_ARG(rows > 0 && rows <= Q_MAXROWS && n > 0 && nq > 0 && nq <= Q_MAXQ, "quantiles: need 1 <= rows <= 64, n > 0, 1 <= nq <= 4");
    QRanks ranks = {};
    for (int i = 0; i < nq; ++i) {
        JP_CHECK_ARG(q[i] >= 0.f && q[i] <= 1.f, "quantiles: q outside [0,1]");
        const long k = std::min<long>((long)std::floor((double)q[i] * (double)(n - 1)), (long)n - 1);
        ranks.k[2 * i] = (unsigned)k;
        ranks.k[2 * i + 1] = (unsigned)std::min<long>(k + 1, (long)n - 1);
    }
    JP_ST;
    unsigned* hist = (unsigned*)ws;
    const size_t pass_words = (size_t)rows * Q_T * Q_BINS;
    QState* state = (QState*)(hist + Q_PASSES * pass_words);
    JP_HIP(hipMemsetAsync(hist, 0, Q_PASSES * pass_words * sizeof(unsigned), st));
    const bool vec = n % 4 == 0 && al16(x);
    const int per_row = std::max(1, std::min(jp_cdiv(vec ? n / 4 : n, TPB * 4), MAX_BLOCKS / rows));
    for (int pass = 0; pass < Q_PASSES; ++pass) {
        unsigned* hp = hist + pass * pass_words;
        if (vec)
            hipLaunchKernelGGL(q_hist_kernel<true>, dim3(per_row, rows), dim3(TPB), 0, st, x, n, state, hp, pass);
        else
            hipLaunchKernelGGL(q_hist_kernel<false>, dim3(per_row, rows), dim3(TPB), 0, st, x, n, state, hp, pass);
        hipLaunchKernelGGL(q_pick_kernel, dim3(rows), dim3(Q_BINS), 0, st, state, hp, pass, 2 * nq, ranks, out);
    }
    JP_LAUNCH_CHECK();
}

// x (rows, n); vmin_vmax (rows, 2) on the device; lut 256 x 3 bytes on the device; out (rows, n, 3) bytes
extern "C" int jp_colorize_u8(const float* x, int rows, int n, const float* vmin_vmax, const uint8_t* lut, uint8_t* out,
                              void* stream) {
    JP_CHECK_ARG(x && vmin_vmax && lut && out, "colorize_u8: null pointer");
    JP_CHECK_ARG(rows > 0 && rows <= 65535 && n > 0, "colorize_u8: need 1 <= rows <= 65535, n > 0");
    JP_ST;
    const bool vec = n % 4 == 0 && al16(x) && al4(out);
    const int per_row = std::max(1, std::min(jp_cdiv(vec ? n / 4 : n, TPB), std::max(1, MAX_BLOCKS / rows)));
    if (vec)
        hipLaunchKernelGGL(colorize_kernel<true>, dim3(per_row, rows), dim3(TPB), 0, st, x, n, vmin_vmax, lut, out);
    else
        hipLaunchKernelGGL(colorize_kernel<false>, dim3(per_row, rows), dim3(TPB), 0, st, x, n, vmin_vmax, lut, out);
    JP_LAUNCH_CHECK();
}

// road_logits / car_logits (B, 2, HW), car_logits nullable; cls (B, HW) bytes 0 = background, 1 = road, 2 = car;
// rgb (nullable) (B, HW, 3) bytes
extern "C" int jp_layout_classes_u8(const float* road_logits, const float* car_logits, uint8_t* cls, uint8_t* rgb, int B, int HW,
                                    void* stream) {
    JP_CHECK_ARG(road_logits && cls, "layout_classes_u8: null pointer");
    JP_CHECK_ARG(B > 0 && B <= 65535 && HW > 0, "layout_classes_u8: need 1 <= B <= 65535, HW > 0");
    JP_ST;
    const bool vec = HW % 4 == 0 && al16(road_logits) && (!car_logits || al16(car_logits)) && al4(cls) && (!rgb || al4(rgb));
    const int per_b = std::max(1, std::min(jp_cdiv(vec ? HW / 4 : HW, TPB), std::max(1, MAX_BLOCKS / B)));
    if (vec)
        hipLaunchKernelGGL(layout_classes_kernel<true>, dim3(per_b, B), dim3(TPB), 0, st, road_logits, car_logits, cls, rgb, HW);
    else
        hipLaunchKernelGGL(layout_classes_kernel<false>, dim3(per_b, B), dim3(TPB), 0, st, road_logits, car_logits, cls, rgb, HW);
    JP_LAUNCH_CHECK();
}
