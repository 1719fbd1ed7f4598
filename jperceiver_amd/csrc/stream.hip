// Streaming perception (apis/stream.py PerceptionStream): the two per-frame kernels of a session that takes camera frames one by one.
// "The previous frame" and "trajectory row k" are not pointer swaps or host-side indices: both kernels read the number of frames pushed
// so far from DEVICE memory (`count`, one int32 of the caller's), so every launch has the same arguments for every frame (what a captured
// graph would need) and nothing is copied back.  The library keeps no state: ring, pose, trajectory and counter are the caller's buffers.
//   jp_stream_pose_pair : resize the new frame to the pose nets' 192 x 640 (jp_bilinear_fwd's arithmetic, bilinear.h), keep it in a
//                         two-slot ring and write the 6-channel pair [previous | new] the PoseEncoder reads -- Baseline.predict_poses'
//                         [pf[-1], pf[0]] for frame_ids = [0, -1] in one launch, the previous frame resized only once.
//   jp_stream_traj_push : pose <- pose @ cam_T_cam in float64 (eval_kitti_video.py:292's chaining), rows 0..2 into the trajectory,
//                         then count <- count + 1.
#include "jp_common.h"
#include "bilinear.h"
#include <algorithm>
#include <climits>

namespace {
constexpr int TPB = 256;
constexpr int PH = 192, PW = 640;            // the pose nets' input (net.py:632)

// One thread per element of the resized frame, lanes along W.  Every thread reads the other ring slot only at the index it writes in
// this slot, so no thread depends on another; `count` is only read.
__global__ __launch_bounds__(TPB) void stream_pose_pair_kernel(const float* __restrict__ frame, float* ring,
                                                               const int* __restrict__ count, float* __restrict__ pair, long total,
                                                               int H, int W, float sy, float sx, unsigned* __restrict__ amax) {
    const int n = *count;
    const int slot = n & 1;
    float* cur = ring + (long)slot * total;
    const float* old = ring + (long)(slot ^ 1) * total;
    float mx = 0.f;
    for (long o = (long)blockIdx.x * TPB + threadIdx.x; o < total; o += (long)gridDim.x * TPB) {
        const int ox = (int)(o % PW);
        const long t = o / PW;
        const int oy = (int)(t % PH);
        const long bc = t / PH;              // b * 3 + c
        const float v = bil_sample(frame + bc * H * W, oy, ox, H, W, sy, sx);
        const float p = n == 0 ? v : old[o]; // the first frame is paired with itself, as the demo does
        cur[o] = v;
        const long b = bc / 3, c = bc - 3 * b;
        float* pp = pair + ((b * 6 + c) * PH + oy) * PW + ox;
        pp[0] = p;
        pp[3L * PH * PW] = v;
        mx = fmaxf(mx, fmaxf(jp_fmag(v), jp_fmag(p)));
    }
    jp_block_amax_commit(mx, amax);
}

// ONE workgroup: 16 threads per camera (one per element of the 4 x 4), 16 cameras per pass.  Every element is
// ((a0 b0 + a1 b1) + a2 b2) + a3 b3 with each product and sum rounded once (no fma).  A pass reads the old poses of its cameras, meets
// at a barrier and only then writes them; the counter is stored by one thread behind the last barrier, when every camera is done.
__global__ __launch_bounds__(TPB) void stream_traj_push_kernel(const float* __restrict__ T, double* pose,
                                                               double* __restrict__ traj, int* __restrict__ count, int B, int capacity) {
    const int n = *count;
    const int e = threadIdx.x & 15, i = e >> 2, j = e & 3;
    for (int b0 = 0; b0 < B; b0 += TPB / 16) {      // (uniform trip count: the barriers are reached by every thread)
        const int b = b0 + (threadIdx.x >> 4);
        double r = i == j ? 1.0 : 0.0;               // n == 0: the identity, whatever T holds
        if (b < B && n != 0) {
            const double* a = pose + (long)b * 16 + i * 4;
            const float* t = T + (long)b * 16 + j;
            r = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(a[0], (double)t[0]), __dmul_rn(a[1], (double)t[4])),
                                    __dmul_rn(a[2], (double)t[8])),
                          __dmul_rn(a[3], (double)t[12]));
        }
        __syncthreads();
        if (b < B) {
            pose[(long)b * 16 + e] = r;
            if (i < 3 && n >= 0 && n < capacity) traj[((long)b * capacity + n) * 12 + e] = r;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *count = n < INT_MAX ? n + 1 : n;
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
// amax_out: optional magnitude slot (see the header) that receives max |pair|
extern "C" int jp_stream_pose_pair(const float* frame, float* ring, const int* count, float* pair, float* amax_out, int B, int H, int W,
                                   void* stream) {
    JP_CHECK_ARG(frame && ring && count && pair, "stream_pose_pair: null pointer");
    JP_CHECK_ARG(B > 0 && H > 0 && W > 0, "stream_pose_pair: B, H and W must be positive");
    JP_CHECK_ARG((long)H * W <= (long)INT_MAX, "stream_pose_pair: H * W must fit an int");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long total = (long)B * 3 * PH * PW;
    const int blocks = (int)std::min<long>((total + TPB - 1) / TPB, 2048);
    hipLaunchKernelGGL(stream_pose_pair_kernel, dim3(blocks), dim3(TPB), 0, st, frame, ring, count, pair, total, H, W,
                       (float)H / (float)PH, (float)W / (float)PW, reinterpret_cast<unsigned*>(amax_out));
    JP_LAUNCH_CHECK();
}

extern "C" int jp_stream_traj_push(const float* T, double* pose, double* traj, int* count, int B, int capacity, void* stream) {
    JP_CHECK_ARG(T && pose && traj && count, "stream_traj_push: null pointer");
    JP_CHECK_ARG(B > 0 && capacity > 0, "stream_traj_push: B and capacity must be positive");
    hipLaunchKernelGGL(stream_traj_push_kernel, dim3(1), dim3(TPB), 0, static_cast<hipStream_t>(stream), T, pose, traj, count, B,
                       capacity);
    JP_LAUNCH_CHECK();
}
