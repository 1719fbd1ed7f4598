// World-frame BEV map (apis/bevmap.py BevMap; PerceptionStream(bev_map=...)): the ego-centred class maps of a drive voted into one map
// with the drive's float64 camera-to-world poses.  The library keeps no state: the vote counts, the class map, the image and the poses are
// the caller's buffers.
//   jp_bev_fuse        : a GATHER.  Every map cell of a fixed-size window around the frame's footprint is taken back into the frame with the
//                        inverse of the pose's x-z block and reads the class of the frame cell it lands in; counts[seen, road, car] += votes.
//   jp_bev_map_classes : vote counts -> class map (255 = not seen often enough) and palette image.
//   jp_bev_map_mark    : paints the map cells a trajectory passes through.
// GEOMETRY.  World is the frame of the first camera pose (T_0 = I); +X goes to increasing map columns, +Z (forward) to decreasing rows, world
// (0, 0) sits at cell coordinates (org_r, org_c): cell (r, c) has its centre at X = (c + 0.5 - org_c) res, Z = (org_r - r - 0.5) res.  Frame
// cell (i, j) covers x in [(j - occ/2) res_f, (j + 1 - occ/2) res_f) and z in [(occ - 1 - i) res_f - off, (occ - i) res_f - off): row i's far
// edge is the forward distance the network's own distance map gives that row.  The BEV plane is taken to be the camera's own x-z plane: only
// rows 0 and 2 of a pose are read, columns 0, 2 and 3 of them, and the shift h R[.][1] that the camera's height above the ground would add is
// dropped.
// ARITHMETIC.  float64, every operation rounded once (no fma contraction), in the order the header states: the result is a pure function of
// the arguments, and tests/bevmap_ref.py restates it operation by operation.  Every range test is written so that NaN fails it, and nothing
// is converted to an integer before the test that bounds it has passed.
#include "jp_common.h"
#include <algorithm>
#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int WX = 64, WY = TPB / WX;          // a workgroup covers 64 map columns (the lanes of a wave) x 4 rows

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

// blockIdx.z = b * N + n.  The window of `win` x `win` map cells is placed by the kernel itself, around the footprint's centre
// T (0, 0, zc): the launch has the same arguments for every frame of a session.  The footprint is the image of a square of side
// occ res_f under the x-z block of a rigid transform (singular values <= 1), so it lies within occ res_f sqrt(2) / 2 of that centre; `win`
// covers that disc with more than a cell to spare on either side.
// ATOMIC = false (N == 1): one thread owns each map cell of a camera, plain read-modify-write.
template <bool ATOMIC>
__global__ __launch_bounds__(TPB) void bev_fuse_kernel(const uint8_t* __restrict__ layout, const double* __restrict__ pose, int pose_stride,
                                                       int N, int* counts, int occ, double res_f, double off, double max_range, int Mh,
                                                       int Mw, double res, double org_r, double org_c, int win, double zc) {
    const int bn = blockIdx.z, b = bn / N;
    const double* T = pose + (long)bn * pose_stride;
    const double t00 = T[0], t02 = T[2], t03 = T[3], t20 = T[8], t22 = T[10], t23 = T[11];
    const double det = dsub(dmul(t00, t22), dmul(t02, t20));
    if (!(fabs(det) >= 1e-6)) return;                                  // singular, NaN: the frame contributes nothing
    // window origin: first row / column, as doubles until they are known to be near the map
    const double half = 0.5 * (double)win;
    const double cc = (t02 * zc + t03) / res + org_c;                  // the centre's continuous column / row coordinate
    const double cr = org_r - (t22 * zc + t23) / res;
    const double fc0 = floor(cc - half), fr0 = floor(cr - half);
    if (!(fc0 > -(double)win - 1.0 && fc0 < (double)Mw && fr0 > -(double)win - 1.0 && fr0 < (double)Mh)) return;   // off the map, NaN, Inf
    const int wc = blockIdx.x * WX + (threadIdx.x & (WX - 1)), wr = blockIdx.y * WY + threadIdx.x / WX;
    if (wc >= win || wr >= win) return;
    const int c = (int)fc0 + wc, r = (int)fr0 + wr;
    if (c < 0 || c >= Mw || r < 0 || r >= Mh) return;
    const double X = dmul(dsub(dadd((double)c, 0.5), org_c), res);
    const double Z = dmul(dsub(dsub(org_r, (double)r), 0.5), res);
    const double dX = dsub(X, t03), dZ = dsub(Z, t23);
    const double x = ddiv(dsub(dmul(t22, dX), dmul(t02, dZ)), det);
    const double z = ddiv(dsub(dmul(t00, dZ), dmul(t20, dX)), det);
    const double u = dadd(ddiv(x, res_f), 0.5 * (double)occ);
    const double v = ddiv(dadd(z, off), res_f);
    const double docc = (double)occ;
    if (!(u >= 0.0 && u < docc && v >= 0.0 && v < docc && z <= max_range)) return;
    const int j = (int)floor(u), i = occ - 1 - (int)floor(v);
    const unsigned cls = layout[((long)bn * occ + i) * occ + j];
    const long cells = (long)Mh * Mw;
    int* p = counts + (long)b * 3 * cells + (long)r * Mw + c;
    if constexpr (ATOMIC) {
        atomicAdd(p, 1);
        if (cls == 1u) atomicAdd(p + cells, 1);
        if (cls == 2u) atomicAdd(p + 2 * cells, 1);
    } else {
        p[0] += 1;
        if (cls == 1u) p[cells] += 1;
        if (cls == 2u) p[2 * cells] += 1;
    }
}

__device__ __forceinline__ unsigned map_rgb(unsigned c) {        // perception.hip's lay_rgb, and (96,96,96) for "not seen"
    return c == 1u ? 0x00ffffffu : (c == 2u ? 0x00ff0000u : (c == 255u ? 0x00606060u : 0u));
}

__global__ __launch_bounds__(TPB) void bev_map_classes_kernel(const int* __restrict__ counts, uint8_t* __restrict__ cls,
                                                              uint8_t* __restrict__ rgb, int cells, double min_seen, double road_frac,
                                                              double car_frac) {
    const int b = blockIdx.y;
    const int* cb = counts + (long)b * 3 * cells;
    for (long k = (long)blockIdx.x * TPB + threadIdx.x; k < cells; k += (long)gridDim.x * TPB) {
        const double seen = (double)cb[k], road = (double)cb[cells + k], car = (double)cb[2L * cells + k];
        unsigned c;
        if (seen < min_seen) c = 255u;
        else if (car >= dmul(car_frac, seen)) c = 2u;
        else if (dadd(road, car) >= dmul(road_frac, seen)) c = 1u;
        else c = 0u;
        const long o = (long)b * cells + k;
        cls[o] = (uint8_t)c;
        if (rgb) {
            const unsigned q = map_rgb(c);
            rgb[3 * o] = (uint8_t)q;
            rgb[3 * o + 1] = (uint8_t)(q >> 8);
            rgb[3 * o + 2] = (uint8_t)(q >> 16);
        }
    }
}

// one thread per trajectory row; rows that land in one cell write the same bytes
__global__ __launch_bounds__(TPB) void bev_map_mark_kernel(uint8_t* rgb, int B, int Mh, int Mw, const double* __restrict__ traj, int n,
                                                           int capacity, double res, double org_r, double org_c, unsigned color) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= B * n) return;
    const int b = t / n, k = t - b * n;
    const double* T = traj + ((long)b * capacity + k) * 12;
    const double fc = floor(dadd(ddiv(T[3], res), org_c));
    const double fr = floor(dsub(org_r, ddiv(T[11], res)));
    if (!(fc >= 0.0 && fc < (double)Mw && fr >= 0.0 && fr < (double)Mh)) return;     // off the map or not finite
    uint8_t* p = rgb + 3 * (((long)b * Mh + (int)fr) * Mw + (int)fc);
    p[0] = (uint8_t)color;
    p[1] = (uint8_t)(color >> 8);
    p[2] = (uint8_t)(color >> 16);
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" int jp_bev_fuse(const uint8_t* layout, const double* pose, int pose_stride, int N, int* counts, int B, int occ, double res_f,
                           double off, double max_range, int Mh, int Mw, double res, double org_r, double org_c, void* stream) {
    JP_CHECK_ARG(layout && pose && counts, "bev_fuse: null pointer");
    JP_CHECK_ARG(B > 0 && N > 0 && occ > 0 && Mh > 0 && Mw > 0, "bev_fuse: B, N, occ, Mh and Mw must be positive");
    JP_CHECK_ARG(pose_stride >= 12, "bev_fuse: pose_stride must be at least 12 (rows 0..2 of a 4 x 4)");
    JP_CHECK_ARG(res > 0.0 && res_f > 0.0, "bev_fuse: res and res_f must be greater than zero");
    JP_CHECK_ARG((long)B * N <= 65535, "bev_fuse: B * N must not exceed 65535");
    const double side = (double)occ * res_f;
    const double w = std::ceil(side * std::sqrt(2.0) / res) + 3.0;
    JP_CHECK_ARG(w <= 32768.0, "bev_fuse: a frame covers more than 32768 map cells a side (res too fine for occ * res_f)");
    const int win = (int)w;
    const dim3 grid(jp_cdiv(win, WX), jp_cdiv(win, WY), B * N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double zc = 0.5 * side - off;                                 // 20 - off for the 40 m layouts
    if (N == 1)
        hipLaunchKernelGGL(bev_fuse_kernel<false>, grid, dim3(TPB), 0, st, layout, pose, pose_stride, N, counts, occ, res_f, off, max_range,
                           Mh, Mw, res, org_r, org_c, win, zc);
    else
        hipLaunchKernelGGL(bev_fuse_kernel<true>, grid, dim3(TPB), 0, st, layout, pose, pose_stride, N, counts, occ, res_f, off, max_range,
                           Mh, Mw, res, org_r, org_c, win, zc);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_bev_map_classes(const int* counts, uint8_t* cls, uint8_t* rgb, int B, int cells, double min_seen, double road_frac,
                                  double car_frac, void* stream) {
    JP_CHECK_ARG(counts && cls, "bev_map_classes: null pointer");
    JP_CHECK_ARG(B > 0 && B <= 65535 && cells > 0, "bev_map_classes: B (<= 65535) and cells must be positive");
    const int blocks = std::min(jp_cdiv(cells, TPB), 2048);
    hipLaunchKernelGGL(bev_map_classes_kernel, dim3(blocks, B), dim3(TPB), 0, static_cast<hipStream_t>(stream), counts, cls, rgb, cells,
                       min_seen, road_frac, car_frac);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_bev_map_mark(uint8_t* rgb, int B, int Mh, int Mw, const double* traj, int n, int capacity, double res, double org_r,
                               double org_c, int color, void* stream) {
    JP_CHECK_ARG(rgb && traj, "bev_map_mark: null pointer");
    JP_CHECK_ARG(B > 0 && Mh > 0 && Mw > 0 && n > 0 && capacity > 0, "bev_map_mark: B, Mh, Mw, n and capacity must be positive");
    JP_CHECK_ARG(n <= capacity, "bev_map_mark: n must not exceed capacity");
    JP_CHECK_ARG((long)B * n <= (long)INT32_MAX, "bev_map_mark: B * n must fit an int");
    JP_CHECK_ARG(res > 0.0, "bev_map_mark: res must be greater than zero");
    hipLaunchKernelGGL(bev_map_mark_kernel, dim3(jp_cdiv((long)B * n, TPB)), dim3(TPB), 0, static_cast<hipStream_t>(stream), rgb, B, Mh,
                       Mw, traj, n, capacity, res, org_r, org_c, (unsigned)color);
    JP_LAUNCH_CHECK();
}
