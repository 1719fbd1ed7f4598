// The ground plane fitted from depth on the device (apis/depthbev.py DepthBev(ground=...); PerceptionStream(depth_bev=dict(ground=...))):
// jp_ground_fit writes [nx, ny, nz, h] into the camera rows jp_depth_bev_lift (depthbev.hip) reads its plane from, so a fit followed by a
// lift needs no host round trip and every launch keeps fixed arguments.  The library keeps no state: depth, layout, prior, camera rows,
// partial sums, moments and status are the caller's buffers, and everything the call leaves is overwritten by it (nothing to zero first).
//   moments kernel : a pure READ of the depth map.  Every pixel is back-projected as the lift does it (the same float64 operations in the
//                    same order: X, Y, d and the cell carry the lift's bits), gated against the current plane (|residual| <= band) and,
//                    with a layout, against the road cells; an accepted pixel is quantised to integer millimetres and adds to ten int64
//                    sums.  Integer sums are exact and order-free: the table is a pure function of the inputs whatever the grid, the wave
//                    order or `parts`.  A workgroup strides over image rows, its lanes run along u; a wave shuffle fold, an LDS fold, one row
//                    of `part` per workgroup -- a workgroup without a pixel stores ten zeros.  No atomics, no workgroup waits on another.
//   solve kernel   : one workgroup per camera folds the `parts` rows in integers, stores them to mom[b], and one thread fits
//                    Y = a X + b Z + c in float64 in the order the header states, every operation rounded once (tests/ground_ref.py
//                    restates it with float64 scalars), applies the status rules and stores the plane or leaves it.
// One call enqueues `rounds` such pairs: round 1 gates with `prior` (or with cam[b][4:8] when prior is null: tracking), later rounds with
// the plane the round before left in cam[b][4:8].
#include "jp_common.h"
#include <cmath>

namespace {
constexpr int TPB = 256, NS = 10, UNROLL = 4;
constexpr int SOLVE_ROWS = 25;                                         // the solve kernel folds the parts as 25 x 10 threads

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (B, parts).  Workgroup (b, p) takes the image rows p, p + parts, ... of camera b, thread t the columns t, t + TPB, ...: the lanes of a
// wave read 64 consecutive floats of one row.
// gate: [nx, ny, nz, h] of camera b at gate + b gate_stride (prior rows: stride 4; the plane inside the camera rows: cam + 4, stride 8).
__global__ __launch_bounds__(TPB) void ground_moments_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ layout,
                                                             const double* __restrict__ gate, int gate_stride,
                                                             const double* __restrict__ cam, long long* __restrict__ part, int H, int W,
                                                             int occ, double res_f, double off, double min_range, double max_range,
                                                             double band) {
    __shared__ long long fold[TPB / 64][NS];
    const int b = blockIdx.x, p = blockIdx.y, parts = gridDim.y;
    const int hw = H * W;                                              // B H W < 2^31
    const float* dep = depth + (long)b * hw;
    const double* c = cam + 8L * b;
    const double* g = gate + (long)gate_stride * b;
    const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
    const double nx = g[0], ny = g[1], nz = g[2], h = g[3];
    const double docc = (double)occ, nband = -band;
    const uint8_t* lay = layout ? layout + (long)b * occ * occ : nullptr;
    long long s[NS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // Rows p, p + parts, ... of the image, UNROLL TPB columns at a time: (u - cx) / fx is formed once per column and kept over the rows,
    // (v - cy) / fy once per row -- the same operations on the same operands as per pixel, so the same bits, at a fraction of the
    // divisions, and no pixel index has to be split into (v, u).
    for (long u0 = 0; u0 < W; u0 += UNROLL * TPB) {
        double xn[UNROLL];
        long col[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; ++j) {
            col[j] = u0 + j * TPB + threadIdx.x;
            xn[j] = ddiv(dsub((double)col[j], cx), fx);
        }
        for (int v = p; v < H; v += parts) {
            const float* row = dep + (long)v * W;
            float f[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j)                               // the loads of a trip are independent: all in flight together
                f[j] = col[j] < W ? row[col[j]] : __int_as_float(0x7fc00000);      // past the row's end: NaN, which the first test rejects
            // The UNROLL pixels of a trip go through every stage together, without branches: a rejected pixel runs along with ok = false
            // and zeros selected in before anything is converted to an integer; a wave with nothing in range (sky) skips the trip.
            double d[UNROLL], X[UNROLL], Y[UNROLL];
            bool ok[UNROLL], any = false;
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                d[j] = (double)f[j];
                ok[j] = d[j] >= min_range && d[j] <= max_range;
                any |= ok[j];
            }
            if (!__any(any)) continue;
            const double yn = ddiv(dsub((double)v, cy), fy);
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                X[j] = dmul(xn[j], d[j]);
                Y[j] = dmul(yn, d[j]);
                const double r = dsub(h, dadd(dadd(dmul(nx, X[j]), dmul(ny, Y[j])), dmul(nz, d[j])));
                ok[j] = ok[j] && fabs(X[j]) <= max_range && fabs(Y[j]) <= max_range && r >= nband && r <= band;
            }
            if (lay) {
#pragma unroll
                for (int j = 0; j < UNROLL; ++j) {
                    const double uu = dadd(ddiv(X[j], res_f), 0.5 * docc);
                    const double vv = ddiv(dadd(d[j], off), res_f);
                    const bool in = ok[j] && uu >= 0.0 && uu < docc && vv >= 0.0 && vv < docc;
                    const int jj = (int)floor(in ? uu : 0.0), ii = occ - 1 - (int)floor(in ? vv : 0.0);
                    ok[j] = in && lay[(long)ii * occ + jj] == 1;           // (a rejected lane reads cell (occ - 1, 0): inside the layout)
                }
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                // |X|, |Y|, d <= max_range <= 1000: the millimetres fit in int32 and their products are 32 x 32 -> 64 multiplies
                const int qx = (int)floor(dadd(dmul(ok[j] ? X[j] : 0.0, 1000.0), 0.5));
                const int qy = (int)floor(dadd(dmul(ok[j] ? Y[j] : 0.0, 1000.0), 0.5));
                const int qz = (int)floor(dadd(dmul(ok[j] ? d[j] : 0.0, 1000.0), 0.5));      // a rejected pixel: 0, 0, 0 -- it adds nothing
                s[0] += ok[j] ? 1 : 0;
                s[1] += qx;
                s[2] += qy;
                s[3] += qz;
                s[4] += (long long)qx * qx;
                s[5] += (long long)qx * qz;
                s[6] += (long long)qz * qz;
                s[7] += (long long)qx * qy;
                s[8] += (long long)qz * qy;
                s[9] += (long long)qy * qy;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) s[i] = wave_sum_ll(s[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) fold[threadIdx.x >> 6][i] = s[i];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) t += fold[w][threadIdx.x];
        part[((long)b * parts + p) * NS + threadIdx.x] = t;
    }
}

// grid (B).  prior: non-null only in round 1 of a call that was given one -- a rejected fit then copies it into cam[b][4:8], so that the
// call alone defines the plane.
__global__ __launch_bounds__(TPB) void ground_solve_kernel(const long long* __restrict__ part, const double* __restrict__ prior,
                                                           double* __restrict__ cam, long long* __restrict__ mom,
                                                           double* __restrict__ stat, int parts, int min_points, double min_spread,
                                                           double cos_tilt, double h_lo, double h_hi) {
    __shared__ long long fold[SOLVE_ROWS][NS];
    __shared__ long long total[NS];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < SOLVE_ROWS * NS) {
        const int row = t / NS, col = t - row * NS;
        const long long* src = part + (long)b * parts * NS;
        long long a = 0;
        for (int r = row; r < parts; r += SOLVE_ROWS) a += src[(long)r * NS + col];
        fold[row][col] = a;
    }
    __syncthreads();
    if (t < NS) {
        long long a = 0;
        for (int r = 0; r < SOLVE_ROWS; ++r) a += fold[r][t];
        total[t] = a;
        mom[(long)b * NS + t] = a;
    }
    __syncthreads();
    if (t != 0) return;
    double* plane = cam + 8L * b + 4;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long long n = total[0];
    int status = 0;
    double out[4] = {nan, nan, nan, nan}, rms = nan;
    if (n < (long long)min_points) {
        status = 1;
    } else {
        const double N = (double)n;
        const double mx = ddiv((double)total[1], N), my = ddiv((double)total[2], N), mz = ddiv((double)total[3], N);
        const double cxx = dsub(ddiv((double)total[4], N), dmul(mx, mx));
        const double cxz = dsub(ddiv((double)total[5], N), dmul(mx, mz));
        const double czz = dsub(ddiv((double)total[6], N), dmul(mz, mz));
        const double cxy = dsub(ddiv((double)total[7], N), dmul(mx, my));
        const double czy = dsub(ddiv((double)total[8], N), dmul(mz, my));
        const double cyy = dsub(ddiv((double)total[9], N), dmul(my, my));
        const double det = dsub(dmul(cxx, czz), dmul(cxz, cxz));
        const double t0 = dmul(1000.0, min_spread), sp = dmul(t0, t0);
        if (!(cxx >= sp && czz >= sp && det >= dmul(0.01, dmul(cxx, czz)))) {
            status = 2;
        } else {
            const double a = ddiv(dsub(dmul(cxy, czz), dmul(czy, cxz)), det);
            const double bb = ddiv(dsub(dmul(czy, cxx), dmul(cxy, cxz)), det);
            const double cc = dsub(my, dadd(dmul(a, mx), dmul(bb, mz)));
            const double s = __dsqrt_rn(dadd(dadd(dmul(a, a), 1.0), dmul(bb, bb)));
            out[0] = ddiv(-a, s);
            out[1] = ddiv(1.0, s);
            out[2] = ddiv(-bb, s);
            out[3] = ddiv(ddiv(cc, 1000.0), s);
            const double e = dsub(cyy, dadd(dmul(a, cxy), dmul(bb, czy)));
            rms = ddiv(ddiv(__dsqrt_rn(e > 0.0 ? e : 0.0), s), 1000.0);
            const bool finite = isfinite(out[0]) && isfinite(out[1]) && isfinite(out[2]) && isfinite(out[3]) && isfinite(rms);
            if (!finite || out[1] < cos_tilt || !(out[3] >= h_lo && out[3] <= h_hi)) status = 3;
        }
    }
    if (status == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) plane[i] = out[i];
    } else if (prior) {
#pragma unroll
        for (int i = 0; i < 4; ++i) plane[i] = prior[4L * b + i];
    }
    stat[3L * b] = (double)status;
    stat[3L * b + 1] = (double)n;
    stat[3L * b + 2] = status == 0 ? rms : nan;
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" int jp_ground_fit(const float* depth, const uint8_t* layout, const double* prior, double* cam, long long* part, long long* mom,
                             double* stat, int B, int H, int W, int occ, double res_f, double off, double min_range, double max_range,
                             double band, int rounds, int parts, int min_points, double min_spread, double max_tilt_deg, double h_lo,
                             double h_hi, void* stream) {
    JP_CHECK_ARG(depth && cam && part && mom && stat, "ground_fit: null pointer (depth, cam, part, mom and stat are required)");
    JP_CHECK_ARG(B > 0 && H > 0 && W > 0 && rounds > 0 && parts > 0, "ground_fit: B, H, W, rounds and parts must be positive");
    JP_CHECK_ARG(parts <= 1024, "ground_fit: parts must not exceed 1024");
    JP_CHECK_ARG(!layout || occ > 0, "ground_fit: occ must be positive when a layout is given");
    JP_CHECK_ARG(res_f > 0.0, "ground_fit: res_f must be greater than zero");
    JP_CHECK_ARG(band > 0.0, "ground_fit: band must be greater than zero");
    JP_CHECK_ARG(max_range > 0.0 && max_range <= 1000.0, "ground_fit: max_range must lie in (0, 1000] (points are kept in int32 millimetres)");
    const double mm = 1000.0 * max_range;
    JP_CHECK_ARG((double)H * (double)W * mm * mm < 4611686018427387904.0,
                 "ground_fit: H * W * (1000 max_range)^2 must be below 2^62 (the int64 sums of squares could overflow)");
    JP_CHECK_ARG((long)B * H * W < (1L << 31), "ground_fit: B * H * W must be below 2^31");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double cos_tilt = std::cos(max_tilt_deg * (M_PI / 180.0));
    for (int r = 0; r < rounds; ++r) {
        const double* first = r == 0 ? prior : nullptr;
        hipLaunchKernelGGL(ground_moments_kernel, dim3(B, parts), dim3(TPB), 0, st, depth, layout, first ? first : cam + 4, first ? 4 : 8, cam,
                           part, H, W, occ, res_f, off, min_range, max_range, band);
        hipLaunchKernelGGL(ground_solve_kernel, dim3(B), dim3(TPB), 0, st, part, first, cam, mom, stat, parts, min_points, min_spread,
                           cos_tilt, h_lo, h_hi);
    }
    JP_LAUNCH_CHECK();
}
