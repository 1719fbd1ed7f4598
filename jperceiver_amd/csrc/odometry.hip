// KITTI odometry evaluation on the device (jperceiver_amd/core/evaluation.py::eval_odometry, apis/inference.py) -- the second half
// of scripts/draw_odometry.py's path, which the reference runs in host numpy on a text file:
//   jp_pose_chain_f64       : global_pose <- global_pose @ inv(T_k) (draw_odometry.py:62-76; without the inverse:
//                             eval_kitti_video.py:292) as an inclusive scan over affine composition
//   jp_odom_segment_errors  : trajectoryDistances + lastFrameFromSegmentLength + calcSequenceErrors
//                             (mono/tools/kitti_evaluation_toolkit.py:109-182)
//   jp_traj_moments         : the sums Umeyama's alignment (mono/tools/geometry.py:38-49), plot_kitti's least-squares scale
//                             (scripts/plot_kitti.py:15-25) and the absolute trajectory error are made of
//   jp_poses_transform_f64  : traj.scale(s) (mono/tools/trajectory.py:162-172) / align_transformation @ pose (plot_kitti.py:240-243)
// All arithmetic is double.  No sum is made with atomics: every fold has a fixed order (a function of n alone), so two runs on the
// same input are bit-identical.  The scans are three launches each (block-local scan, one workgroup over the block aggregates,
// apply): no workgroup ever waits on another.  These are latency-bound kernels of a few thousand elements; a pose is 12 doubles
// (96 bytes), so a thread that owns a pose reads / writes one contiguous 96-byte piece and a wave covers one contiguous range.
#include "jp_common.h"
#include <algorithm>

namespace {
constexpr int TPB = 256;             // scan block width: 4 waves of 64
constexpr int MOM_BLOCKS = 64;       // partial sums of jp_traj_moments: at most one wave's worth, folded by lane
constexpr int MAX_LEN = 16;          // segment lengths per call

// ------------------------------------------------------------------ affine maps [R | t] as 12 doubles, row-major 3x4
// general inverse: adjugate over the determinant, then -A^-1 t (NOT the transpose: a float32 Rodrigues matrix is orthonormal only
// to ~1e-7, and that error would be carried along the whole chain)
__device__ __forceinline__ void aff_inverse(const double* m, double* o) {
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
    const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double inv = 1.0 / (a * c00 + b * c10 + c * c20);
    o[0] = c00 * inv, o[1] = c01 * inv, o[2] = c02 * inv;
    o[4] = c10 * inv, o[5] = c11 * inv, o[6] = c12 * inv;
    o[8] = c20 * inv, o[9] = c21 * inv, o[10] = c22 * inv;
    const double tx = m[3], ty = m[7], tz = m[11];
    o[3] = -(o[0] * tx + o[1] * ty + o[2] * tz);
    o[7] = -(o[4] * tx + o[5] * ty + o[6] * tz);
    o[11] = -(o[8] * tx + o[9] * ty + o[10] * tz);
}
// o = a . b  (o may not alias a or b)
__device__ __forceinline__ void aff_mul(const double* a, const double* b, double* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[4 * r + c] = a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c] + a[4 * r + 2] * b[8 + c];
        o[4 * r + 3] += a[4 * r + 3];
    }
}

// the two monoids that are scanned: affine composition (earlier . later) and the plain sum
struct AffOp {
    static constexpr int NC = 12;
    static __device__ __forceinline__ void identity(double* v) {
#pragma unroll
        for (int c = 0; c < 12; ++c) v[c] = (c == 0 || c == 5 || c == 10) ? 1.0 : 0.0;
    }
    static __device__ __forceinline__ void combine(const double* earlier, double* later) {      // later <- earlier . later
        double o[12];
        aff_mul(earlier, later, o);
#pragma unroll
        for (int c = 0; c < 12; ++c) later[c] = o[c];
    }
};
struct AddOp {
    static constexpr int NC = 1;
    static __device__ __forceinline__ void identity(double* v) { v[0] = 0.0; }
    static __device__ __forceinline__ void combine(const double* earlier, double* later) { later[0] = earlier[0] + later[0]; }
};

// inclusive scan of one element per thread over the workgroup (Hillis-Steele, log2(TPB) steps).  sm: Op::NC * TPB doubles, one
// row per component (lane l of a wave reads bytes 8 l .. 8 l + 7 of a row: no bank conflict).  On return v holds the thread's
// result and sm the results of all threads; ends with a barrier.
template <class Op>
__device__ __forceinline__ void block_scan(double* v, double* sm) {
    constexpr int NC = Op::NC;
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < NC; ++c) sm[c * TPB + tid] = v[c];
    __syncthreads();
    for (int o = 1; o < TPB; o <<= 1) {
        double p[NC];
        if (tid >= o) {
#pragma unroll
            for (int c = 0; c < NC; ++c) p[c] = sm[c * TPB + tid - o];
        }
        __syncthreads();
        if (tid >= o) {
            Op::combine(p, v);
#pragma unroll
            for (int c = 0; c < NC; ++c) sm[c * TPB + tid] = v[c];
        }
        __syncthreads();
    }
}

// launch 2 of a scan: ONE workgroup turns the nb block aggregates into their inclusive scan, in place; more than TPB of them are
// taken TPB at a time with a carry (any n works)
template <class Op>
__global__ __launch_bounds__(TPB) void scan_aggregates_kernel(double* __restrict__ agg, int nb) {
    constexpr int NC = Op::NC;
    __shared__ double sm[NC * TPB];
    const int tid = threadIdx.x;
    double carry[NC];
    Op::identity(carry);
    for (int base = 0; base < nb; base += TPB) {
        const int i = base + tid;
        double v[NC];
        Op::identity(v);
        if (i < nb) {
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = agg[(size_t)i * NC + c];
        }
        block_scan<Op>(v, sm);
        Op::combine(carry, v);
        if (i < nb) {
#pragma unroll
            for (int c = 0; c < NC; ++c) agg[(size_t)i * NC + c] = v[c];
        }
        if (tid == TPB - 1) {
#pragma unroll
            for (int c = 0; c < NC; ++c) sm[c] = v[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) carry[c] = sm[c];
        __syncthreads();
    }
}

// launch 3 of a scan: element i of block b >= 1 becomes (scan of the aggregates)[b - 1] . element.  out points at element 0
template <class Op>
__global__ __launch_bounds__(TPB) void scan_apply_kernel(double* __restrict__ out, const double* __restrict__ agg, int n) {
    constexpr int NC = Op::NC;
    const int b = blockIdx.x + 1;
    const long i = (long)b * TPB + threadIdx.x;
    if (i >= n) return;
    double p[NC], v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = agg[(size_t)(b - 1) * NC + c];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = out[(size_t)i * NC + c];
    Op::combine(p, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) out[(size_t)i * NC + c] = v[c];
}

// launch 1 of the pose chain: M_k = T_k or its inverse, scanned inside the block; poses row k + 1 <- the block-local product,
// agg[block] <- the product of the whole block.  T is (n,4,4) float, row 3 is not read.
__global__ __launch_bounds__(TPB) void chain_local_kernel(const float* __restrict__ T, int n, int invert,
                                                          double* __restrict__ poses, double* __restrict__ agg) {
    __shared__ double sm[12 * TPB];
    const int tid = threadIdx.x;
    const long k = (long)blockIdx.x * TPB + tid;
    double v[12];
    AffOp::identity(v);
    if (k < n) {
        double m[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = (double)T[(size_t)k * 16 + c];
        if (invert) {
            aff_inverse(m, v);
        } else {
#pragma unroll
            for (int c = 0; c < 12; ++c) v[c] = m[c];
        }
    }
    block_scan<AffOp>(v, sm);
    // the block's rows are one contiguous piece of `poses`: written element by element from the LDS copy, lane l next to lane l + 1
    const long first = (long)blockIdx.x * TPB;
    const int cnt = (n - first < TPB ? (int)(n - first) : TPB) * 12;
    double* dst = poses + (size_t)(first + 1) * 12;
    for (int j = tid; j < cnt; j += TPB) dst[j] = sm[(j % 12) * TPB + j / 12];
    if (blockIdx.x == 0 && tid < 12) poses[tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
    if (tid == TPB - 1) {               // threads past n hold the identity: the last thread has the product of the valid ones
#pragma unroll
        for (int c = 0; c < 12; ++c) agg[(size_t)blockIdx.x * 12 + c] = v[c];
    }
}

// launch 1 of trajectoryDistances: dist[0] = 0, dist[i] = dist[i-1] + |p_{i-1} - p_i| (kitti_evaluation_toolkit.py:109-126)
__global__ __launch_bounds__(TPB) void dist_local_kernel(const double* __restrict__ gt, int n, double* __restrict__ dist,
                                                         double* __restrict__ agg) {
    __shared__ double sm[TPB];
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    double v[1] = {0.0};
    if (i > 0 && i < n) {
        const double* p1 = gt + (size_t)(i - 1) * 12;
        const double* p2 = p1 + 12;
        const double dx = p1[3] - p2[3], dy = p1[7] - p2[7], dz = p1[11] - p2[11];
        v[0] = sqrt(dx * dx + dy * dy + dz * dz);
    }
    block_scan<AddOp>(v, sm);
    if (i < n) dist[i] = v[0];
    if (threadIdx.x == TPB - 1) agg[blockIdx.x] = v[0];
}

struct OdomLengths { double v[MAX_LEN]; };

__device__ __forceinline__ void load_pose(const double* __restrict__ p, double* m) {
#pragma unroll
    for (int c = 0; c < 12; ++c) m[c] = p[c];
}

// one thread per (start frame, length): lastFrameFromSegmentLength by bisection (dist is non-decreasing, so the first frame past
// the target is the one the reference's linear scan stops at), then calcSequenceErrors' row (:147-182)
__global__ __launch_bounds__(TPB) void segment_errors_kernel(const double* __restrict__ gt, const double* __restrict__ pred, int n,
                                                             int step, OdomLengths lengths, int nlen, int total,
                                                             const double* __restrict__ dist, int* __restrict__ last_frame,
                                                             double* __restrict__ table) {
    const int idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= total) return;
    const int s = idx / nlen, l = idx - s * nlen;
    const long first = (long)s * step;                       // < n: s < ceil(n / step)
    const double len = lengths.v[l];
    const double target = dist[first] + len;
    long lo = first, hi = n;                                 // first i in [first, n) with dist[i] > target, n if none
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (dist[mid] > target) hi = mid; else lo = mid + 1;
    }
    if (lo >= n) {
        last_frame[idx] = -1;
        return;
    }
    const int last = (int)lo;
    last_frame[idx] = last;
    double a[12], b[12], ia[12], dg[12], dr[12], err[12];
    load_pose(gt + (size_t)first * 12, a);
    load_pose(gt + (size_t)last * 12, b);
    aff_inverse(a, ia);
    aff_mul(ia, b, dg);                                      // pose_delta_gt
    load_pose(pred + (size_t)first * 12, a);
    load_pose(pred + (size_t)last * 12, b);
    aff_inverse(a, ia);
    aff_mul(ia, b, dr);                                      // pose_delta_result
    aff_inverse(dr, ia);
    aff_mul(ia, dg, err);                                    // pose_error
    const double d = 0.5 * (err[0] + err[5] + err[10] - 1.0);
    const double r_err = acos(d > 1.0 ? 1.0 : (d < -1.0 ? -1.0 : d));
    const double t_err = sqrt(err[3] * err[3] + err[7] * err[7] + err[11] * err[11]);
    const double num_frames = (double)(last - first) + 1.0;
    double* row = table + (size_t)idx * 5;
    row[0] = (double)first;
    row[1] = r_err / len;
    row[2] = t_err / len;
    row[3] = len;
    row[4] = len / (0.1 * num_frames);
}

// ------------------------------------------------------------------ trajectory moments: means first, then centred sums
__device__ __forceinline__ void load_pos(const double* __restrict__ p, long i, double* v) {
    v[0] = p[(size_t)i * 12 + 3], v[1] = p[(size_t)i * 12 + 7], v[2] = p[(size_t)i * 12 + 11];
}

// part1[block][0..5] = the block's share of sum x, sum y
__global__ __launch_bounds__(TPB) void moments_sums_kernel(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                           double* __restrict__ part1) {
    __shared__ double sm[4];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
        double px[3], py[3];
        load_pos(x, i, px);
        load_pos(y, i, py);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += px[k], acc[3 + k] += py[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double s = jp_block_sum_d(acc[k], sm);
        if (threadIdx.x == 0) part1[blockIdx.x * 6 + k] = s;
    }
}

// the fold of the per-block partials, by one wave: lane b holds block b's (nb <= 64), the xor butterfly adds them in one fixed
// order and leaves the total in every lane
template <int K>
__device__ __forceinline__ void fold_partials(const double* __restrict__ part, int nb, double* out) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = jp_wave_sum_d(lane < nb ? part[lane * K + k] : 0.0);
}

// part2[block][0..12] = the block's share of sum |x-mx|^2, sum (y-my)(x-mx)^T (9, row-major), sum x.y, sum x.x, sum |x-y|^2;
// every block folds the means from part1 itself, the same way: all of them (and the finishing launch) get the same bits
__global__ __launch_bounds__(TPB) void moments_centred_kernel(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                              const double* __restrict__ part1, int nb1,
                                                              double* __restrict__ part2) {
    __shared__ double sm[4];
    __shared__ double mean[6];
    if (threadIdx.x < 64) {
        double m[6];
        fold_partials<6>(part1, nb1, m);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) mean[k] = m[k] / (double)n;
        }
    }
    __syncthreads();
    double mx[3] = {mean[0], mean[1], mean[2]}, my[3] = {mean[3], mean[4], mean[5]};
    double acc[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0.0;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
        double px[3], py[3];
        load_pos(x, i, px);
        load_pos(y, i, py);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double cx = px[r] - mx[r], d = px[r] - py[r];
            acc[0] += cx * cx;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[1 + 3 * r + c] += (py[r] - my[r]) * (px[c] - mx[c]);
            acc[10] += px[r] * py[r];
            acc[11] += px[r] * px[r];
            acc[12] += d * d;
        }
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const double s = jp_block_sum_d(acc[k], sm);
        if (threadIdx.x == 0) part2[blockIdx.x * 13 + k] = s;
    }
}

// one wave: out[0..5] = means, out[6] = sigma_x^2, out[7..15] = cov, out[16..18] = sum x.y, sum x.x, sum |x-y|^2
__global__ __launch_bounds__(64) void moments_finish_kernel(const double* __restrict__ part1, const double* __restrict__ part2,
                                                            int nb, int n, double* __restrict__ out) {
    double m[6], s[13];
    fold_partials<6>(part1, nb, m);
    fold_partials<13>(part2, nb, s);
    if (threadIdx.x == 0) {
        const double dn = (double)n;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = m[k] / dn;
#pragma unroll
        for (int k = 0; k < 10; ++k) out[6 + k] = s[k] / dn;
        out[16] = s[10], out[17] = s[11], out[18] = s[12];
    }
}

struct Aff12 { double v[12]; };

// out_k = A . [R_k | scale t_k]; a thread owns a pose and reads all of it before it writes, so out may be poses
__global__ __launch_bounds__(TPB) void poses_transform_kernel(const double* poses, int n, Aff12 A, double scale, double* out) {
    for (long k = (long)blockIdx.x * TPB + threadIdx.x; k < n; k += (long)gridDim.x * TPB) {
        double m[12], o[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) m[c] = poses[(size_t)k * 12 + c];
        m[3] *= scale, m[7] *= scale, m[11] *= scale;
        aff_mul(A.v, m, o);
#pragma unroll
        for (int c = 0; c < 12; ++c) out[(size_t)k * 12 + c] = o[c];
    }
}

inline int moments_blocks(int n) { return std::min(jp_cdiv(n, TPB), MOM_BLOCKS); }
}  // namespace

#define JP_ST hipStream_t st = (hipStream_t)stream

// bytes of caller scratch for jp_pose_chain_f64 on n transforms (need not be initialised)
extern "C" long jp_pose_chain_ws_bytes(int n) {
    JP_CHECK_ARG(n > 0, "pose_chain_ws_bytes: n must be positive");
    return (long)jp_cdiv(n, TPB) * 12 * (long)sizeof(double);
}

// T (n,4,4) float frame-to-frame transforms (row 3 is not read: taken as 0 0 0 1) -> poses (n+1,12): rows 0..2 of G_0 = I,
// G_k = G_{k-1} . M_k with M_k = T_k^-1 (invert != 0; the general affine inverse) or T_k
extern "C" int jp_pose_chain_f64(const float* T, int n, int invert, double* poses, void* ws, void* stream) {
    JP_CHECK_ARG(T && poses && ws, "pose_chain_f64: null pointer");
    JP_CHECK_ARG(n > 0, "pose_chain_f64: n must be positive");
    JP_ST;
    const int nb = jp_cdiv(n, TPB);
    double* agg = (double*)ws;
    hipLaunchKernelGGL(chain_local_kernel, dim3(nb), dim3(TPB), 0, st, T, n, invert, poses, agg);
    if (nb > 1) {
        hipLaunchKernelGGL(scan_aggregates_kernel<AffOp>, dim3(1), dim3(TPB), 0, st, agg, nb - 1);
        hipLaunchKernelGGL(scan_apply_kernel<AffOp>, dim3(nb - 1), dim3(TPB), 0, st, poses + 12, (const double*)agg, n);
    }
    JP_LAUNCH_CHECK();
}

// bytes of caller scratch for jp_odom_segment_errors (need not be initialised)
extern "C" long jp_odom_segments_ws_bytes(int n, int step, int nlen) {
    JP_CHECK_ARG(n > 0 && step > 0 && nlen >= 1 && nlen <= MAX_LEN, "odom_segments_ws_bytes: need n > 0, step > 0, 1 <= nlen <= 16");
    return (long)jp_cdiv(n, TPB) * (long)sizeof(double);
}

// gt / pred (n,12) poses; lengths: HOST array of nlen <= 16 positive segment lengths in metres; dist (n): cumulative ground-truth
// path length; with S = ceil(n / step) start frames s * step: last_frame (S * nlen) = first i >= first with
// dist[i] > dist[first] + len, or -1; table (S * nlen, 5) rows [first_frame, r_err / len, t_err / len, len, speed], untouched where
// last_frame is -1
extern "C" int jp_odom_segment_errors(const double* gt, const double* pred, int n, int step, const double* lengths, int nlen,
                                      double* dist, int* last_frame, double* table, void* ws, void* stream) {
    JP_CHECK_ARG(gt && pred && lengths && dist && last_frame && table && ws, "odom_segment_errors: null pointer");
    JP_CHECK_ARG(n > 0, "odom_segment_errors: n must be positive");
    JP_CHECK_ARG(step > 0, "odom_segment_errors: step must be positive");
    JP_CHECK_ARG(nlen >= 1 && nlen <= MAX_LEN, "odom_segment_errors: nlen must be 1..16");
    OdomLengths L = {};
    for (int i = 0; i < nlen; ++i) {
        JP_CHECK_ARG(lengths[i] > 0.0, "odom_segment_errors: segment lengths must be positive");
        L.v[i] = lengths[i];
    }
    const long total = (long)jp_cdiv(n, step) * nlen;
    JP_CHECK_ARG(total <= 0x7fffffffL, "odom_segment_errors: too many segments");
    JP_ST;
    const int nb = jp_cdiv(n, TPB);
    double* agg = (double*)ws;
    hipLaunchKernelGGL(dist_local_kernel, dim3(nb), dim3(TPB), 0, st, gt, n, dist, agg);
    if (nb > 1) {
        hipLaunchKernelGGL(scan_aggregates_kernel<AddOp>, dim3(1), dim3(TPB), 0, st, agg, nb - 1);
        hipLaunchKernelGGL(scan_apply_kernel<AddOp>, dim3(nb - 1), dim3(TPB), 0, st, dist, (const double*)agg, n);
    }
    hipLaunchKernelGGL(segment_errors_kernel, dim3(jp_cdiv(total, TPB)), dim3(TPB), 0, st, gt, pred, n, step, L, nlen, (int)total,
                       (const double*)dist, last_frame, table);
    JP_LAUNCH_CHECK();
}

// bytes of caller scratch for jp_traj_moments (need not be initialised)
extern "C" long jp_traj_moments_ws_bytes(int n) {
    JP_CHECK_ARG(n > 0, "traj_moments_ws_bytes: n must be positive");
    return (long)moments_blocks(n) * (6 + 13) * (long)sizeof(double);
}

// x / y (n,12) poses, of which the positions (columns 3, 7, 11) are read -> out (19): mean_x (3), mean_y (3),
// sigma_x^2 = 1/n sum |x - mean_x|^2, cov = 1/n sum (y - mean_y)(x - mean_x)^T (9, row-major), sum x.y, sum x.x, sum |x - y|^2
extern "C" int jp_traj_moments(const double* x, const double* y, int n, double* out, void* ws, void* stream) {
    JP_CHECK_ARG(x && y && out && ws, "traj_moments: null pointer");
    JP_CHECK_ARG(n > 0, "traj_moments: n must be positive");
    JP_ST;
    const int nb = moments_blocks(n);
    double* part1 = (double*)ws;
    double* part2 = part1 + (size_t)nb * 6;
    hipLaunchKernelGGL(moments_sums_kernel, dim3(nb), dim3(TPB), 0, st, x, y, n, part1);
    hipLaunchKernelGGL(moments_centred_kernel, dim3(nb), dim3(TPB), 0, st, x, y, n, (const double*)part1, nb, part2);
    hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)part1, (const double*)part2, nb, n, out);
    JP_LAUNCH_CHECK();
}

// out_k = A . [R_k | scale t_k] for n poses (n,12); A: HOST array of 12 doubles (rows 0..2 of a 4x4).  A = I is traj.scale(scale),
// exactly; out may be poses
extern "C" int jp_poses_transform_f64(const double* poses, int n, const double* A, double scale, double* out, void* stream) {
    JP_CHECK_ARG(poses && A && out, "poses_transform_f64: null pointer");
    JP_CHECK_ARG(n > 0, "poses_transform_f64: n must be positive");
    Aff12 a;
    for (int c = 0; c < 12; ++c) a.v[c] = A[c];
    JP_ST;
    hipLaunchKernelGGL(poses_transform_kernel, dim3(std::min(jp_cdiv(n, TPB), 1024)), dim3(TPB), 0, st, poses, n, a, scale, out);
    JP_LAUNCH_CHECK();
}
