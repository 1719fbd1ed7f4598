// Depth lifted into the layout's BEV grid, and the agreement of the two heads (apis/depthbev.py DepthBev; PerceptionStream(depth_bev=...)):
// the inverse of the training-time warp (jp_scale_label_assemble takes the BEV distance map into the image), on the frame-cell geometry of
// jp_bev_fuse (bevmap.hip).  The library keeps no state: depth, camera rows, grid, class maps and counts are the caller's buffers.
//   jp_depth_bev_lift    : a SCATTER.  Every pixel is back-projected with its depth, given a height above the caller's ground plane and
//                          dropped into the cell it stands over; grid[n, n_obst, hmin_mm, hmax_mm] is updated with integer atomics.
//   jp_depth_bev_classes : grid -> class map (255 not observed, 1 ground, 2 obstacle) and height map.
//   jp_bev_agree         : 2 x 3 table of lifted class against layout class, per camera.
// ARITHMETIC of the lift.  float64, every operation rounded once (no fma contraction), in the order the header states: the result is a pure
// function of the arguments, and tests/depthbev_ref.py restates it operation by operation.  Every range test is written so that NaN fails
// it, and nothing is converted to an integer before the test that bounds it has passed.  Integer add / min / max do not depend on the order
// of arrival: two runs give the same bits.
// TWO FORMS of the lift (JP_DEPTH_BEV_RUNS, read at every call; default: see depth_bev_runs() below).  Lanes run along an image row, so
// neighbouring lanes mostly hit the same cell.  RUNS = false: every accepted lane issues its own atomics.  RUNS = true: a wave folds each
// run of equal cell keys with a segmented log-step scan and only the last lane of a run issues atomics; a rejected lane carries key -1,
// which ends a run and issues nothing.  Both forms give the same grid.
#include "jp_common.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

namespace {
constexpr int TPB = 256;

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

// planes [n, n_obst, hmin_mm, hmax_mm] of every camera: the neutral element of the lift's updates
__global__ __launch_bounds__(TPB) void depth_bev_fill_kernel(int* __restrict__ grid, int cells, long total) {
    for (long k = (long)blockIdx.x * TPB + threadIdx.x; k < total; k += (long)gridDim.x * TPB) {
        const int plane = (int)((k / cells) & 3);
        grid[k] = plane < 2 ? 0 : (plane == 2 ? INT_MAX : INT_MIN);
    }
}

// One thread per pixel, pixels in memory order: the lanes of a wave are 64 consecutive u of one image row (or the end of one row and the
// start of the next).  No thread leaves before the wave's shuffles: a pixel past the end is a rejected lane.
template <bool RUNS>
__global__ __launch_bounds__(TPB) void depth_bev_lift_kernel(const float* __restrict__ depth, const double* __restrict__ cam, int* grid,
                                                             long total, int H, int W, int occ, double res_f, double off,
                                                             double min_range, double max_range, double h_min, double h_max,
                                                             double obst_h) {
    const long p = (long)blockIdx.x * TPB + threadIdx.x;
    const int cells = occ * occ;
    int key = -1, q = 0, ob = 0, b = 0;                                // key: cell index within the camera's planes, -1 = rejected
    if (p < total) {
        const long hw = (long)H * W;
        b = (int)(p / hw);
        const int rem = (int)(p - (long)b * hw);
        const int v = rem / W, u = rem - v * W;
        const double* c = cam + 8L * b;
        const double d = (double)depth[p];
        if (d >= min_range && d <= max_range) {
            const double X = dmul(ddiv(dsub((double)u, c[2]), c[0]), d);
            const double Y = dmul(ddiv(dsub((double)v, c[3]), c[1]), d);
            const double hgt = dsub(c[7], dadd(dadd(dmul(c[4], X), dmul(c[5], Y)), dmul(c[6], d)));
            if (hgt >= h_min && hgt <= h_max) {
                const double docc = (double)occ;
                const double uu = dadd(ddiv(X, res_f), 0.5 * docc);
                const double vv = ddiv(dadd(d, off), res_f);
                if (uu >= 0.0 && uu < docc && vv >= 0.0 && vv < docc) {
                    const int j = (int)floor(uu), i = occ - 1 - (int)floor(vv);
                    key = i * occ + j;
                    q = (int)floor(dadd(dmul(hgt, 1000.0), 0.5));
                    ob = hgt > obst_h ? 1 : 0;
                }
            }
        }
    }
    if constexpr (!RUNS) {
        if (key < 0) return;
        int* g = grid + (long)b * 4 * cells + key;
        atomicAdd(g, 1);
        if (ob) atomicAdd(g + cells, 1);
        atomicMin(g + 2 * cells, q);
        atomicMax(g + 3 * cells, q);
    } else {
        // a run = consecutive lanes with the same (camera, cell); the camera only changes where p crosses a multiple of H W, so the pair is
        // compared as one 64-bit word
        const int lane = threadIdx.x & 63;
        const long long id = key < 0 ? -1LL : (long long)b * cells + key;
        const long long before = __shfl_up(id, 1, 64);
        const bool head = lane == 0 || before != id;
        const unsigned long long heads = __ballot(head);
        const int start = 63 - __clzll((long long)(heads & (~0ULL >> (63 - lane))));       // first lane of this lane's run
        int n = 1, mn = q, mx = q;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                              // inclusive scan over [start, lane]
            const int n2 = __shfl_up(n, o, 64), ob2 = __shfl_up(ob, o, 64), mn2 = __shfl_up(mn, o, 64), mx2 = __shfl_up(mx, o, 64);
            if (lane - o >= start) {
                n += n2;
                ob += ob2;
                mn = min(mn, mn2);
                mx = max(mx, mx2);
            }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ULL);
        if (key < 0 || !tail) return;
        int* g = grid + (long)b * 4 * cells + key;
        atomicAdd(g, n);
        if (ob) atomicAdd(g + cells, ob);
        atomicMin(g + 2 * cells, mn);
        atomicMax(g + 3 * cells, mx);
    }
}

__global__ __launch_bounds__(TPB) void depth_bev_classes_kernel(const int* __restrict__ grid, uint8_t* __restrict__ cls,
                                                                float* __restrict__ height, int cells, int min_points, int obst_points) {
    const int b = blockIdx.y;
    const int* g = grid + (long)b * 4 * cells;
    for (long k = (long)blockIdx.x * TPB + threadIdx.x; k < cells; k += (long)gridDim.x * TPB) {
        const int n = g[k], no = g[cells + k];
        const unsigned c = n < min_points ? 255u : (no >= obst_points ? 2u : 1u);
        const long o = (long)b * cells + k;
        cls[o] = (uint8_t)c;
        if (height) height[o] = c == 255u ? __int_as_float(0x7fc00000) : __fdiv_rn((float)g[3L * cells + k], 1000.0f);
    }
}

// One workgroup per camera sweeps its cells and stores the six counts: nothing to zero first, no atomics, no workgroup waits on another.
constexpr int ATPB = 1024;
__global__ __launch_bounds__(ATPB) void bev_agree_kernel(const uint8_t* __restrict__ lifted, const uint8_t* __restrict__ layout,
                                                         int* __restrict__ out, int cells) {
    __shared__ int part[ATPB / 64][6];
    const int b = blockIdx.x;
    const uint8_t* a = lifted + (long)b * cells;
    const uint8_t* l = layout + (long)b * cells;
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int k = threadIdx.x; k < cells; k += ATPB) {
        const unsigned x = a[k], c = l[k];
        if ((x == 1u || x == 2u) && c <= 2u) {
            const unsigned slot = (x - 1u) * 3u + c;
#pragma unroll
            for (unsigned s = 0; s < 6; ++s) cnt[s] += slot == s;
        }
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int v = cnt[s];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        cnt[s] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 6; ++s) part[threadIdx.x >> 6][s] = cnt[s];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int v = 0;
        for (int w = 0; w < ATPB / 64; ++w) v += part[w][threadIdx.x];
        out[b * 6 + threadIdx.x] = v;
    }
}

// JP_DEPTH_BEV_RUNS=0 / 1 picks the form of the lift; read at every call so that one process can run both.  Default: the run
// aggregation, the faster of the two on the road scene of tools/depthbev_bench.py (profiles/depth_bev.md).
bool depth_bev_runs() {
    const char* e = getenv("JP_DEPTH_BEV_RUNS");
    return !(e && e[0] == '0');
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" int jp_depth_bev_lift(const float* depth, const double* cam, int* grid, int B, int H, int W, int occ, double res_f, double off,
                                 double min_range, double max_range, double h_min, double h_max, double obst_h, int accumulate,
                                 void* stream) {
    JP_CHECK_ARG(depth && cam && grid, "depth_bev_lift: null pointer");
    JP_CHECK_ARG(B > 0 && H > 0 && W > 0 && occ > 0, "depth_bev_lift: B, H, W and occ must be positive");
    JP_CHECK_ARG(res_f > 0.0, "depth_bev_lift: res_f must be greater than zero");
    JP_CHECK_ARG(std::fabs(h_min) <= 1e6 && std::fabs(h_max) <= 1e6, "depth_bev_lift: |h_min| and |h_max| must not exceed 1e6 (heights are kept in int32 millimetres)");
    const long total = (long)B * H * W;
    JP_CHECK_ARG(total < (1L << 31), "depth_bev_lift: B * H * W must be below 2^31");
    const long gtotal = (long)B * 4 * occ * occ;
    JP_CHECK_ARG(gtotal < (1L << 31), "depth_bev_lift: B * 4 * occ * occ must be below 2^31");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!accumulate) {
        const int blocks = std::min(jp_cdiv(gtotal, TPB), 2048);
        hipLaunchKernelGGL(depth_bev_fill_kernel, dim3(blocks), dim3(TPB), 0, st, grid, occ * occ, gtotal);
    }
    const dim3 blocks(jp_cdiv(total, TPB));
    if (depth_bev_runs())
        hipLaunchKernelGGL(depth_bev_lift_kernel<true>, blocks, dim3(TPB), 0, st, depth, cam, grid, total, H, W, occ, res_f, off, min_range,
                           max_range, h_min, h_max, obst_h);
    else
        hipLaunchKernelGGL(depth_bev_lift_kernel<false>, blocks, dim3(TPB), 0, st, depth, cam, grid, total, H, W, occ, res_f, off, min_range,
                           max_range, h_min, h_max, obst_h);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_depth_bev_classes(const int* grid, uint8_t* cls, float* height, int B, int cells, int min_points, int obst_points,
                                    void* stream) {
    JP_CHECK_ARG(grid && cls, "depth_bev_classes: null pointer");
    JP_CHECK_ARG(B > 0 && B <= 65535 && cells > 0, "depth_bev_classes: B (<= 65535) and cells must be positive");
    JP_CHECK_ARG((long)B * 4 * cells < (1L << 31), "depth_bev_classes: B * 4 * cells must be below 2^31");
    const int blocks = std::min(jp_cdiv(cells, TPB), 2048);
    hipLaunchKernelGGL(depth_bev_classes_kernel, dim3(blocks, B), dim3(TPB), 0, static_cast<hipStream_t>(stream), grid, cls, height, cells,
                       min_points, obst_points);
    JP_LAUNCH_CHECK();
}

extern "C" int jp_bev_agree(const uint8_t* lifted, const uint8_t* layout, int* out, int B, int cells, void* stream) {
    JP_CHECK_ARG(lifted && layout && out, "bev_agree: null pointer");
    JP_CHECK_ARG(B > 0 && cells > 0, "bev_agree: B and cells must be positive");
    hipLaunchKernelGGL(bev_agree_kernel, dim3(B), dim3(ATPB), 0, static_cast<hipStream_t>(stream), lifted, layout, out, cells);
    JP_LAUNCH_CHECK();
}
