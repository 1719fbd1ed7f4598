// Filtered BEV tracks (apis/bevfilter.py BevTrackFilter; PerceptionStream(objects=dict(track=dict(filter=...)))): a stage BEHIND jp_bev_tracks
// that gives its frame-to-frame tracks a life cycle (tentative -> confirmed -> coasting -> ended), an id that survives missed frames and
// id switches of the tracker, and a constant-velocity Kalman filter per world axis.  It reads only what jp_bev_tracks wrote (tracks, kin,
// stats), never a label map.  The library keeps no state: the filter's slots live in buffers of the caller that the call rolls forward.
// ONE launch with fixed arguments, grid (B): one workgroup per camera, one thread per slot and per object (both <= 256), no global
// atomics, no workspace, no workgroup waits on another.
//   objects  : thread c reads object c (range-checked against stats), its measurement and the used flags go to LDS.
//   predict  : thread s, in registers.
//   continue : thread s looks its src_track up among the objects' track ids (ids are only compared).
//   re-acquire: greedy rounds.  A candidate slot keeps its nearest free object within the gate (its d^2 recomputed from LDS only when that
//              object was taken by another slot: the S x M matrix is never stored); a round is one min-reduction over the bit pattern
//              of the non-negative d^2, ties to the smaller slot (the slot's own scan has already settled ties to the smaller object).
//   births   : two prefix sums -- the unbound objects in id order, the slots free at entry in slot order -- pair them up.
//   update / miss / status: thread s, in registers; every slot row is written once at the end.
// ARITHMETIC.  float64, every operation rounded once (no fma contraction), in the order the header states: the result is a pure function
// of the arguments and the state, two runs give the same bytes.  tests/bevfilter_ref.py restates it operation by operation.
#include "jp_common.h"
#include <cfloat>
#include <cmath>

namespace {
constexpr int FTPB = 256;                                              // one thread per slot and per object: max_tracks, max_objects <= 256
constexpr int NI = 8, ND = 10;                                         // words of a row of slots_i, doubles of a row of slots_d
typedef unsigned long long u64;
constexpr u64 NONE = ~0ULL;                                            // no pair within the gate (above the bits of every double >= 0)

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ bool fin(double a) { return fabs(a) <= DBL_MAX; }                        // false for NaN and +-Inf
__device__ __forceinline__ int clamp0(int v, int hi) { return min(max(v, 0), hi); }

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = ((u64)(unsigned)__shfl_xor((int)(v >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// one axis of the prediction: p' = p + v; a' = ((a + (b + b)) + c) + q/4, b' = (b + c) + q/2, c' = c + q
__device__ __forceinline__ void predict(double& p, const double v, double& a, double& b, double& c, double q, double q2, double q4) {
    p = dadd(p, v);
    a = dadd(dadd(dadd(a, dadd(b, b)), c), q4);
    b = dadd(dadd(b, c), q2);
    c = dadd(c, q);
}

// one axis of the update from the predicted state with the measurement z
__device__ __forceinline__ void update(double& p, double& v, double& a, double& b, double& c, double z, double r) {
    const double y = dsub(z, p), sx = dadd(a, r), k1 = ddiv(a, sx), k2 = ddiv(b, sx);
    p = dadd(p, dmul(k1, y));
    v = dadd(v, dmul(k2, y));
    const double a0 = a, b0 = b;
    a = dsub(a0, dmul(k1, a0));
    b = dsub(b0, dmul(k1, b0));
    c = dsub(c, dmul(k2, b0));
}

// grid (B), FTPB threads.  Thread tid is slot tid (tid < S) and object tid (tid < n <= M); every LDS index is tid or a value below n or S.
__global__ __launch_bounds__(FTPB) void bevfilter_kernel(const int* __restrict__ tracks, const double* __restrict__ kin,
                                                         const int* __restrict__ stats, int* slots_i, double* slots_d, int* head,
                                                         int* __restrict__ obj_slot, int* __restrict__ fstats, int M, int S, int max_coast,
                                                         int min_hits, double gate2, double r, double c0, double q, double q2, double q4) {
    __shared__ double mX[FTPB], mZ[FTPB];                              // the measurements
    __shared__ int ot[FTPB], ofree[FTPB], oslot[FTPB];                 // per object: its track id, valid and not yet bound, its slot
    __shared__ int pick[FTPB], flist[FTPB], blist[FTPB];               // per slot: the object it continues; the free slots; the births
    __shared__ u64 wkey[FTPB / 64];
    __shared__ int wslot[FTPB / 64], wobj[FTPB / 64], wcnt[FTPB / 64][8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 below = (1ULL << lane) - 1ULL;
    const int n = clamp0(stats[(long)b * 4], M);                       // the tracker's word: never trusted beyond M
    // ---- 0. the objects
    int t = 0;
    double zx = 0.0, zz = 0.0;
    bool valid = false;
    if (tid < n) {
        t = tracks[((long)b * M + tid) * 4];
        zx = kin[((long)b * M + tid) * 4];
        zz = kin[((long)b * M + tid) * 4 + 1];
        valid = fin(zx) && fin(zz);
    }
    ot[tid] = t;
    mX[tid] = zx;
    mZ[tid] = zz;
    ofree[tid] = valid ? 1 : 0;
    oslot[tid] = -1;
    // ---- 1. the slots: predict the live ones
    int si[NI];
    double sd[ND];
#pragma unroll
    for (int f = 0; f < NI; ++f) si[f] = 0;
#pragma unroll
    for (int f = 0; f < ND; ++f) sd[f] = 0.0;
    int* srow_i = slots_i + ((long)b * S + tid) * NI;
    double* srow_d = slots_d + ((long)b * S + tid) * ND;
    if (tid < S) {
#pragma unroll
        for (int f = 0; f < NI; ++f) si[f] = srow_i[f];
#pragma unroll
        for (int f = 0; f < ND; ++f) sd[f] = srow_d[f];
    }
    const bool live = tid < S && si[1] >= 1 && si[1] <= 3, free0 = tid < S && !live;
    if (live) {
        predict(sd[0], sd[2], sd[4], sd[5], sd[6], q, q2, q4);
        predict(sd[1], sd[3], sd[7], sd[8], sd[9], q, q2, q4);
    }
    const int next_fid = head[(long)b * 2], calls = head[(long)b * 2 + 1];
    __syncthreads();
    // ---- 2. continue: the slot picks the smallest valid object that carries its src_track, the object the smallest slot that picked it
    int p = -1;
    if (live && si[5] == 0)
        for (int c = 0; c < n; ++c)
            if (ofree[c] && ot[c] == si[2]) {
                p = c;
                break;
            }
    pick[tid] = p;
    __syncthreads();
    if (valid)
        for (int s = 0; s < S; ++s)
            if (pick[s] == tid) {
                oslot[tid] = s;
                ofree[tid] = 0;
                break;
            }
    __syncthreads();
    const bool cont = p >= 0 && oslot[p] == tid;
    int myobj = cont ? p : -1;                                         // the object whose measurement this slot takes
    // ---- 3. re-acquire: greedy, the smallest d^2 first, ties to the smaller slot, then the smaller object
    bool cand = live && !cont, need = true, reacq = false;
    u64 bd = NONE;
    int bc = -1;
    const int rounds = min(S, n);
    for (int rd = 0; rd < rounds; ++rd) {
        if (cand && need) {
            bd = NONE;
            bc = -1;
            for (int c = 0; c < n; ++c) {
                if (!ofree[c]) continue;
                const double dx = dsub(mX[c], sd[0]), dz = dsub(mZ[c], sd[1]);
                const double d2 = dadd(dmul(dx, dx), dmul(dz, dz));
                if (!(d2 <= gate2)) continue;                          // NaN fails
                const u64 bits = (u64)__double_as_longlong(d2);        // d2 >= +0: the order of the bits is the order of the values
                if (bits < bd) {                                       // strictly: ties stay with the smaller object
                    bd = bits;
                    bc = c;
                }
            }
            need = false;
        }
        const u64 k = cand ? bd : NONE, wm = wave_min(k);
        const u64 at = __ballot(k == wm);                              // never empty
        if (lane == __ffsll((long long)at) - 1) {                      // the smallest slot of the wave that holds the minimum
            wkey[w] = wm;
            wslot[w] = tid;
            wobj[w] = bc;
        }
        __syncthreads();
        u64 best = wkey[0];
        int bw = 0;
#pragma unroll
        for (int i = 1; i < FTPB / 64; ++i)
            if (wkey[i] < best) {                                      // strictly: ties stay with the smaller slot
                best = wkey[i];
                bw = i;
            }
        if (best == NONE) break;                                       // uniform: no pair is left within the gate
        const int ws = wslot[bw], wc = wobj[bw];                       // ws < S, 0 <= wc < n
        if (tid == ws) {
            cand = false;
            reacq = true;
            myobj = wc;
        }
        if (tid == wc) {
            ofree[tid] = 0;
            oslot[tid] = ws;
        }
        if (bc == wc) need = true;                                     // its nearest object is gone: scan again
        __syncthreads();
    }
    __syncthreads();
    // ---- 4. births: the k-th unbound object in id order takes the k-th slot that was free at entry
    const bool birth = valid && ofree[tid] != 0;
    const u64 bm = __ballot(birth), fm = __ballot(free0);
    if (lane == 0) {
        wcnt[w][0] = __popcll(bm);
        wcnt[w][1] = __popcll(fm);
    }
    __syncthreads();
    int brank = __popcll(bm & below), frank = __popcll(fm & below), nbirth = 0, nfree = 0;
#pragma unroll
    for (int i = 0; i < FTPB / 64; ++i) {
        brank += i < w ? wcnt[i][0] : 0;
        frank += i < w ? wcnt[i][1] : 0;
        nbirth += wcnt[i][0];
        nfree += wcnt[i][1];
    }
    if (birth) blist[brank] = tid;                                     // brank < nbirth <= n
    if (free0) flist[frank] = tid;                                     // frank < nfree <= S
    __syncthreads();
    if (birth) oslot[tid] = brank < nfree ? flist[brank] : -1;
    const int born = min(nbirth, nfree);
    const bool isborn = free0 && frank < nbirth;
    if (isborn) {
        myobj = blist[frank];
        si[0] = next_fid + frank;
        si[2] = ot[myobj];
        si[3] = si[4] = 1;
        si[5] = 0;
        sd[0] = mX[myobj];
        sd[1] = mZ[myobj];
        sd[2] = sd[3] = sd[5] = sd[8] = 0.0;
        sd[4] = sd[7] = r;
        sd[6] = sd[9] = c0;
    }
    // ---- 5. update, 6. miss, 7. status
    bool ended = false;
    if (live && myobj >= 0) {
        update(sd[0], sd[2], sd[4], sd[5], sd[6], mX[myobj], r);
        update(sd[1], sd[3], sd[7], sd[8], sd[9], mZ[myobj], r);
        si[2] = ot[myobj];                                             // a re-acquired slot is rebound; a continued one holds it already
        si[3] += 1;
        si[4] += 1;
        si[5] = 0;
    } else if (live) {
        if (si[1] == 1 || si[5] >= max_coast) {                       // misses + 1 > max_coast
            ended = true;
#pragma unroll
            for (int f = 0; f < NI; ++f) si[f] = 0;
#pragma unroll
            for (int f = 0; f < ND; ++f) sd[f] = 0.0;
        } else {
            si[5] += 1;
            si[3] += 1;
            si[1] = 3;
            si[6] = -1;
        }
    }
    if (myobj >= 0) {
        si[1] = si[4] >= min_hits ? 2 : 1;
        si[6] = myobj;
        si[7] = 0;
    }
    if (tid < S && !live && !isborn) {                                 // not live at exit: the row is zero whatever it held
#pragma unroll
        for (int f = 0; f < NI; ++f) si[f] = 0;
#pragma unroll
        for (int f = 0; f < ND; ++f) sd[f] = 0.0;
    }
    if (tid < S) {
#pragma unroll
        for (int f = 0; f < NI; ++f) srow_i[f] = si[f];
#pragma unroll
        for (int f = 0; f < ND; ++f) srow_d[f] = sd[f];
    }
    if (tid < M) obj_slot[(long)b * M + tid] = oslot[tid];
    const u64 m0 = __ballot(si[1] != 0), m1 = __ballot(si[1] == 2), m2 = __ballot(si[1] == 3), m3 = __ballot(cont), m4 = __ballot(reacq),
              m5 = __ballot(ended);
    if (lane == 0) {
        wcnt[w][2] = __popcll(m0);
        wcnt[w][3] = __popcll(m1);
        wcnt[w][4] = __popcll(m2);
        wcnt[w][5] = __popcll(m3);
        wcnt[w][6] = __popcll(m4);
        wcnt[w][7] = __popcll(m5);
    }
    __syncthreads();
    if (tid == 0) {
        int sum[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < FTPB / 64; ++i)
            for (int f = 0; f < 6; ++f) sum[f] += wcnt[i][2 + f];
        int* fo = fstats + (long)b * 8;
        fo[0] = sum[0];
        fo[1] = sum[1];
        fo[2] = sum[2];
        fo[3] = sum[3];
        fo[4] = sum[4];
        fo[5] = born;
        fo[6] = sum[5];
        fo[7] = nbirth - born;
        head[(long)b * 2] = next_fid + born;
        head[(long)b * 2 + 1] = calls + 1;
    }
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" int jp_bev_track_filter(const int* tracks, const double* kin, const int* stats, int* slots_i, double* slots_d, int* head,
                                   int* obj_slot, int* fstats, int B, int max_objects, int max_tracks, int max_coast, int min_hits,
                                   double gate, double meas_sigma, double vel_sigma0, double accel_sigma, void* stream) {
    JP_CHECK_ARG(tracks && kin && stats && slots_i && slots_d && head && obj_slot && fstats,
                 "bev_track_filter: null pointer (tracks, kin, stats, slots_i, slots_d, head, obj_slot and fstats are required)");
    JP_CHECK_ARG(B > 0 && max_objects > 0 && max_tracks > 0, "bev_track_filter: B, max_objects and max_tracks must be positive");
    JP_CHECK_ARG(max_objects <= 256, "bev_track_filter: max_objects must not exceed 256 (the limit of jp_bev_tracks, whose rows it reads)");
    JP_CHECK_ARG(max_tracks <= 256, "bev_track_filter: max_tracks must not exceed 256 (one thread of the camera's workgroup per slot)");
    JP_CHECK_ARG(max_coast >= 0, "bev_track_filter: max_coast must not be negative");
    JP_CHECK_ARG(min_hits >= 1, "bev_track_filter: min_hits must be at least 1");
    JP_CHECK_ARG(std::isfinite(gate) && gate >= 0.0, "bev_track_filter: gate must be finite and not negative");
    JP_CHECK_ARG(std::isfinite(meas_sigma) && meas_sigma > 0.0, "bev_track_filter: meas_sigma must be finite and greater than zero");
    JP_CHECK_ARG(std::isfinite(vel_sigma0) && vel_sigma0 >= 0.0, "bev_track_filter: vel_sigma0 must be finite and not negative");
    JP_CHECK_ARG(std::isfinite(accel_sigma) && accel_sigma >= 0.0, "bev_track_filter: accel_sigma must be finite and not negative");
    JP_CHECK_ARG((long)B * max_tracks * ND < (1L << 31), "bev_track_filter: B * max_tracks * 10 must be below 2^31");
    JP_CHECK_ARG((long)B * max_objects * 4 < (1L << 31), "bev_track_filter: B * max_objects * 4 must be below 2^31");
    // each squared once, one rounded multiply (the host compiler contracts nothing here: every product stands alone)
    const double gate2 = gate * gate, r = meas_sigma * meas_sigma, c0 = vel_sigma0 * vel_sigma0, q = accel_sigma * accel_sigma;
    const double q2 = q * 0.5, q4 = q * 0.25;
    hipLaunchKernelGGL(bevfilter_kernel, dim3(B), dim3(FTPB), 0, static_cast<hipStream_t>(stream), tracks, kin, stats, slots_i, slots_d, head,
                       obj_slot, fstats, max_objects, max_tracks, max_coast, min_hits, gate2, r, c0, q, q2, q4);
    JP_LAUNCH_CHECK();
}
