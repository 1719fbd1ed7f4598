// BEV object tracks (apis/bevtrack.py BevTracker; PerceptionStream(objects=dict(track=...))): the objects of jp_bev_objects associated from
// one frame to the next by cell overlap under the ego-motion, so that a vehicle keeps one track id while it stays in view.  The library
// keeps no state: the previous frame (its label map, its pose, its objects' track ids, ages and world positions) lives in three buffers
// of the caller that every call reads and, as its last step, rolls forward.  One call enqueues FOUR launches with fixed arguments; a phase
// that needs a global order is a launch of its own: no workgroup waits on another (no grid barrier, no flag, no cooperative launch).
//   zero   : the overlap matrix (B, M, M) in ws.
//   vote   : one thread per cell of the CURRENT label map.  A cell of object c is carried to the world with the current pose and back
//            into the previous camera with the stored pose (the planar inverse of bev_fuse_kernel); every cell of the previous label map
//            within `reach` of where it lands that holds a previous object p votes overlap[p][c] += 1.  Votes are folded before they
//            reach global memory (bev_tracks_vote() below): lanes run along a map row, neighbouring lanes mostly carry the same (p, c).
//   assign : one workgroup per camera.  Greedy: the largest overlap among unused rows and columns, ties to the smaller p, then the
//            smaller c, by a max-reduction of a packed 64-bit key, at most min(n_prev, n_cur) rounds; then births in id order by a
//            prefix sum, the outputs, and the roll of the per-object state and the pose.
//   roll   : the current label map becomes the stored one.
// ARITHMETIC.  float64, every operation rounded once (no fma contraction), in the order the header states; integer atomics for the votes:
// the result is a pure function of the arguments and two runs give the same bytes.  Every range test is written so that NaN fails it, and
// nothing is converted to an integer before the test that bounds it has passed.  tests/bevtrack_ref.py restates it operation by operation.
#include "jp_common.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

namespace {
constexpr int TPB = 256;
constexpr int VTPB = 1024;                                             // cells per workgroup of the vote
constexpr int ATPB = 256;                                              // the assignment: one thread per table row (max_objects <= 256)
constexpr int KEEP = 16;                                               // pairs of the matrix a thread of the assignment keeps in registers
constexpr int TILE_M = 64;                                             // largest max_objects whose matrix a workgroup keeps in LDS (16 KB)
constexpr int NF = 12;                                                 // words of a row of jp_bev_objects' table
typedef unsigned long long u64;

__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ bool fin(double a) { return fabs(a) <= DBL_MAX; }                        // false for NaN and +-Inf
__device__ __forceinline__ int clamp0(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(TPB) void bevtrack_zero_kernel(int* __restrict__ p, int n) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) p[i] = 0;
}

__global__ __launch_bounds__(TPB) void bevtrack_roll_kernel(const int* __restrict__ labels, int* __restrict__ prev_labels, int n) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) prev_labels[i] = labels[i];
}

// blockIdx.x = b * bpc + chunk: a workgroup's VTPB cells belong to one camera.
// MODE 0: every vote is a global atomicAdd of 1.  MODE 1: a wave folds each run of consecutive lanes with the same (p, c) and the run's
// first lane adds its length.  MODE 2 (M <= TILE_M): the same runs go to a tile of the camera's matrix in LDS, and the workgroup adds
// the tile's non-zero words to global memory once.  Integer sums: the three give the same matrix.
template <int MODE>
__global__ __launch_bounds__(VTPB) void bevtrack_vote_kernel(const int* __restrict__ labels, const double* __restrict__ pose, int pose_stride,
                                                             const int* __restrict__ prev_labels, const int* __restrict__ state_i,
                                                             const double* __restrict__ state_d, int* overlap, int bpc, int occ,
                                                             int cells, int M, int reach, double res_f, double off) {
    __shared__ int tile[MODE == 2 ? TILE_M * TILE_M : 1];
    const int b = blockIdx.x / bpc, chunk = blockIdx.x - b * bpc;
    // everything up to the first barrier is uniform over the workgroup
    const int n_prev = clamp0(state_i[(long)b * (2 + 2 * M)], M);      // the caller's word: never trusted as an index bound beyond M
    if (n_prev == 0) return;                                           // no history: no votes
    const double* T = pose + (long)b * pose_stride;
    const double* P = state_d + (long)b * (12 + 2 * M);
    const double t00 = T[0], t02 = T[2], t03 = T[3], t20 = T[8], t22 = T[10], t23 = T[11];
    const double p00 = P[0], p02 = P[2], p03 = P[3], p20 = P[8], p22 = P[10], p23 = P[11];
    const double det = dsub(dmul(p00, p22), dmul(p02, p20));
    if (!(fabs(det) >= 1e-6)) return;                                  // singular, NaN: no votes
    if (!(fin(t00) && fin(t02) && fin(t03) && fin(t20) && fin(t22) && fin(t23))) return;
    if (MODE == 2) {
        for (int i = threadIdx.x; i < M * M; i += VTPB) tile[i] = 0;
        __syncthreads();
    }
    const int k = chunk * VTPB + threadIdx.x, lane = threadIdx.x & 63;
    int c = -1, i0 = 0, j0 = 0;
    bool hit = false;
    if (k < cells) {
        c = labels[b * cells + k];
        if (c < 0 || c >= M) c = -1;                                   // background, dropped, or an id beyond the table: not tracked
    }
    if (c >= 0) {
        const int i = k / occ, j = k - i * occ;
        const double docc = (double)occ, hocc = 0.5 * docc;
        const double x = dmul(dsub(dadd((double)j, 0.5), hocc), res_f);
        const double z = dsub(dmul(dsub(dsub(docc, 0.5), (double)i), res_f), off);
        const double X = dadd(dadd(dmul(t00, x), dmul(t02, z)), t03);
        const double Z = dadd(dadd(dmul(t20, x), dmul(t22, z)), t23);
        const double dX = dsub(X, p03), dZ = dsub(Z, p23);
        const double xp = ddiv(dsub(dmul(p22, dX), dmul(p02, dZ)), det);
        const double zp = ddiv(dsub(dmul(p00, dZ), dmul(p20, dX)), det);
        const double u = dadd(ddiv(xp, res_f), hocc);
        const double v = ddiv(dadd(zp, off), res_f);
        if (u >= 0.0 && u < docc && v >= 0.0 && v < docc) {
            hit = true;
            j0 = (int)floor(u);
            i0 = occ - 1 - (int)floor(v);
        }
    }
    if (__ballot(hit)) {                                               // uniform over the wave: the ballots below see all of it
        const int* pl = prev_labels + b * cells;
        int* ov = overlap + (long)b * M * M;
        for (int di = -reach; di <= reach; ++di)
            for (int dj = -reach; dj <= reach; ++dj) {
                int key = -1;
                const int ii = i0 + di, jj = j0 + dj;
                if (hit && ii >= 0 && ii < occ && jj >= 0 && jj < occ) {
                    const int p = pl[ii * occ + jj];
                    if (p >= 0 && p < n_prev) key = p * M + c;         // < M * M
                }
                if (MODE == 0) {
                    if (key >= 0) atomicAdd(ov + key, 1);
                } else {
                    const int before = __shfl_up(key, 1, 64);
                    const bool head = lane == 0 || before != key;
                    const u64 heads = __ballot(head);
                    if (head && key >= 0) {
                        const u64 rest = lane == 63 ? 0ULL : heads >> (lane + 1);
                        const int len = rest ? __ffsll((long long)rest) : 64 - lane;       // lanes up to the next head
                        atomicAdd(MODE == 2 ? &tile[key] : ov + key, len);
                    }
                }
            }
    }
    if (MODE == 2) {
        __syncthreads();
        int* ov = overlap + (long)b * M * M;
        for (int i = threadIdx.x; i < M * M; i += VTPB) {
            const int v = tile[i];
            if (v) atomicAdd(ov + i, v);
        }
    }
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = ((u64)(unsigned)__shfl_xor((int)(v >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// grid (B).  key = overlap << 32 | (65535 - p) << 16 | (65535 - c): the maximum is the largest overlap, then the smaller p, then the
// smaller c -- the pair the sequential loop takes next.  A round scans what is left of the n_prev x n_cur corner of the matrix.
__global__ __launch_bounds__(ATPB) void bevtrack_assign_kernel(const int* __restrict__ count, const int* __restrict__ table,
                                                               const double* __restrict__ pose, int pose_stride, int* state_i,
                                                               double* state_d, const int* __restrict__ overlap, int* __restrict__ tracks,
                                                               double* __restrict__ kin, int* __restrict__ stats, int occ, int M,
                                                               int min_overlap, double res_f, double off) {
    __shared__ u64 wbest[ATPB / 64];
    __shared__ int row_used[ATPB], col_p[ATPB], col_ov[ATPB], wsum[ATPB / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int* si = state_i + (long)b * (2 + 2 * M);
    double* sd = state_d + (long)b * (12 + 2 * M);
    const double* T = pose + (long)b * pose_stride;
    const int n_prev = clamp0(si[0], M), next_id = si[1], n_cur = clamp0(count[b], M);
    const int* ov = overlap + (long)b * M * M;
    row_used[tid] = 0;
    col_p[tid] = -1;                                                   // the previous object a current one is matched to
    col_ov[tid] = 0;
    __syncthreads();
    const int pairs = n_prev * n_cur, rounds = min(n_prev, n_cur);
    // up to KEEP pairs per thread (64 x 64 objects: all of them) are loaded once and stay in registers: a round then waits for no load
    int kv[KEEP], kpc[KEEP];
    const bool kept = pairs <= ATPB * KEEP;
#pragma unroll
    for (int t = 0; t < KEEP; ++t) {
        const int q = tid + t * ATPB;
        kv[t] = 0;
        kpc[t] = 0;
        if (kept && q < pairs) {
            const int p = q / n_cur, c = q - p * n_cur, v = ov[p * M + c];
            kv[t] = v >= min_overlap ? v : 0;                          // min_overlap >= 1: 0 = never a candidate
            kpc[t] = (p << 16) | c;
        }
    }
    int matched = 0;
    for (int r = 0; r < rounds; ++r) {
        u64 best = 0ULL;
        if (kept) {
#pragma unroll
            for (int t = 0; t < KEEP; ++t) {
                const int p = kpc[t] >> 16, c = kpc[t] & 0xffff;
                if (kv[t] == 0 || row_used[p] || col_p[c] >= 0) continue;
                const u64 key = ((u64)(unsigned)kv[t] << 32) | ((u64)(65535 - p) << 16) | (u64)(65535 - c);
                best = key > best ? key : best;
            }
        } else {
            for (int q = tid; q < pairs; q += ATPB) {
                const int p = q / n_cur, c = q - p * n_cur;
                if (row_used[p] || col_p[c] >= 0) continue;
                const int v = ov[p * M + c];
                if (v < min_overlap) continue;                         // min_overlap >= 1: a key is never 0
                const u64 key = ((u64)(unsigned)v << 32) | ((u64)(65535 - p) << 16) | (u64)(65535 - c);
                best = key > best ? key : best;
            }
        }
        best = wave_max(best);
        if (lane == 0) wbest[w] = best;
        __syncthreads();
        best = wbest[0];
#pragma unroll
        for (int i = 1; i < ATPB / 64; ++i) best = wbest[i] > best ? wbest[i] : best;
        if (best == 0ULL) break;                                       // uniform: nothing left at or above min_overlap
        if (tid == 0) {
            const int p = 65535 - (int)((best >> 16) & 0xffffULL), c = 65535 - (int)(best & 0xffffULL);
            row_used[p] = 1;
            col_p[c] = p;
            col_ov[c] = (int)(best >> 32);
        }
        ++matched;
        __syncthreads();
    }
    // births take ids in ascending object id: an exclusive prefix sum over the rows
    const int mine = tid < n_cur ? col_p[tid] : -1;
    const bool birth = tid < n_cur && mine < 0;
    const u64 bm = __ballot(birth);
    if (lane == 0) wsum[w] = __popcll(bm);
    // what a matched object inherits is read before any row of the state is written
    int ptrack = 0, page = 0;
    double pX = 0.0, pZ = 0.0;
    if (mine >= 0) {
        ptrack = si[2 + 2 * mine];
        page = si[3 + 2 * mine];
        pX = sd[12 + 2 * mine];
        pZ = sd[13 + 2 * mine];
    }
    __syncthreads();
    int rank = __popcll(bm & ((1ULL << lane) - 1ULL)), born = 0;
#pragma unroll
    for (int i = 0; i < ATPB / 64; ++i) {
        rank += i < w ? wsum[i] : 0;
        born += wsum[i];
    }
    if (tid < M) {
        int tr[4] = {-1, 0, -1, 0};
        double kn[4] = {0.0, 0.0, 0.0, 0.0};
        int s_track = 0, s_age = 0;
        if (tid < n_cur) {
            const int* row = table + ((long)b * M + tid) * NF;
            const double n = (double)row[0], sr = (double)row[5], sc = (double)row[6];
            const double docc = (double)occ, hocc = 0.5 * docc;
            const double x = dmul(dsub(dadd(ddiv(sc, n), 0.5), hocc), res_f);
            const double z = dsub(dmul(dsub(dsub(docc, 0.5), ddiv(sr, n)), res_f), off);
            kn[0] = dadd(dadd(dmul(T[0], x), dmul(T[2], z)), T[3]);
            kn[1] = dadd(dadd(dmul(T[8], x), dmul(T[10], z)), T[11]);
            if (mine >= 0) {
                tr[0] = ptrack;
                tr[1] = page + 1;
                tr[2] = mine;
                tr[3] = col_ov[tid];
                kn[2] = dsub(kn[0], pX);
                kn[3] = dsub(kn[1], pZ);
            } else {
                tr[0] = next_id + rank;
                tr[1] = 1;
            }
            s_track = tr[0];
            s_age = tr[1];
        }
        int* to = tracks + ((long)b * M + tid) * 4;
        double* ko = kin + ((long)b * M + tid) * 4;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            to[f] = tr[f];
            ko[f] = kn[f];
        }
        si[2 + 2 * tid] = s_track;                                     // rows at or beyond n_cur: zero
        si[3 + 2 * tid] = s_age;
        sd[12 + 2 * tid] = kn[0];
        sd[13 + 2 * tid] = kn[1];
    }
    if (tid < 12) sd[tid] = T[tid];
    if (tid == 0) {
        si[0] = n_cur;
        si[1] = next_id + born;
        int* so = stats + (long)b * 4;
        so[0] = n_cur;
        so[1] = matched;
        so[2] = born;
        so[3] = n_prev - matched;
    }
}

// JP_BEV_TRACKS_VOTE=0 / 1 / 2 picks the form of the vote (MODE above); read at every call so that one process can run all three.
// Default: the LDS tile where the matrix fits one (max_objects <= 64), the wave-local runs above that (profiles/bev_tracks.md).
int bev_tracks_vote(int M) {
    const char* e = getenv("JP_BEV_TRACKS_VOTE");
    int mode = M <= TILE_M ? 2 : 1;
    if (e && e[0] >= '0' && e[0] <= '2' && e[1] == 0) mode = e[0] - '0';
    return mode == 2 && M > TILE_M ? 1 : mode;
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" long jp_bev_tracks_ws_bytes(int B, int occ, int max_objects) {
    if (B <= 0 || occ <= 0 || max_objects <= 0) return 0;
    return (long)sizeof(int) * B * max_objects * max_objects;          // the overlap matrix
}

extern "C" int jp_bev_tracks(const int* labels, const int* count, const int* table, const double* pose, int pose_stride, int* prev_labels,
                             int* state_i, double* state_d, int* tracks, double* kin, int* stats, void* ws, int B, int occ,
                             int max_objects, int reach, int min_overlap, double off, void* stream) {
    JP_CHECK_ARG(labels && count && table && pose && prev_labels && state_i && state_d && tracks && kin && stats && ws,
                 "bev_tracks: null pointer (labels, count, table, pose, prev_labels, state_i, state_d, tracks, kin, stats and ws are required)");
    JP_CHECK_ARG(B > 0 && occ > 0 && max_objects > 0, "bev_tracks: B, occ and max_objects must be positive");
    JP_CHECK_ARG(occ <= 1024, "bev_tracks: occ must not exceed 1024 (the limit of jp_bev_objects, whose table it reads)");
    JP_CHECK_ARG(max_objects <= 256,
                 "bev_tracks: max_objects must not exceed 256 (the overlap matrix and the rounds of the assignment grow with its square)");
    JP_CHECK_ARG(reach >= 0 && reach <= 3, "bev_tracks: reach must lie in 0 .. 3");
    JP_CHECK_ARG(min_overlap >= 1, "bev_tracks: min_overlap must be at least 1");
    JP_CHECK_ARG(pose_stride == 12 || pose_stride == 16, "bev_tracks: pose_stride must be 12 or 16 (rows 0..2 of a 4 x 4, or all of it)");
    JP_CHECK_ARG(std::isfinite(off), "bev_tracks: off must be finite");
    JP_CHECK_ARG((long)B * occ * occ < (1L << 31), "bev_tracks: B * occ * occ must be below 2^31");
    JP_CHECK_ARG((long)B * max_objects * max_objects < (1L << 31), "bev_tracks: B * max_objects * max_objects must be below 2^31");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int M = max_objects, cells = occ * occ, total = B * cells, nov = B * M * M;
    const double res_f = 40.0 / (double)occ;
    int* overlap = static_cast<int*>(ws);
    hipLaunchKernelGGL(bevtrack_zero_kernel, dim3(std::min(jp_cdiv(nov, TPB), 1024)), dim3(TPB), 0, st, overlap, nov);
    const int bpc = jp_cdiv(cells, VTPB);                              // B * bpc <= B * occ * occ < 2^31
    const dim3 vgrid(B * bpc);
    switch (bev_tracks_vote(M)) {
        case 0:
            hipLaunchKernelGGL(bevtrack_vote_kernel<0>, vgrid, dim3(VTPB), 0, st, labels, pose, pose_stride, prev_labels, state_i, state_d,
                               overlap, bpc, occ, cells, M, reach, res_f, off);
            break;
        case 1:
            hipLaunchKernelGGL(bevtrack_vote_kernel<1>, vgrid, dim3(VTPB), 0, st, labels, pose, pose_stride, prev_labels, state_i, state_d,
                               overlap, bpc, occ, cells, M, reach, res_f, off);
            break;
        default:
            hipLaunchKernelGGL(bevtrack_vote_kernel<2>, vgrid, dim3(VTPB), 0, st, labels, pose, pose_stride, prev_labels, state_i, state_d,
                               overlap, bpc, occ, cells, M, reach, res_f, off);
    }
    hipLaunchKernelGGL(bevtrack_assign_kernel, dim3(B), dim3(ATPB), 0, st, count, table, pose, pose_stride, state_i, state_d, overlap, tracks,
                       kin, stats, occ, M, min_overlap, res_f, off);
    hipLaunchKernelGGL(bevtrack_roll_kernel, dim3(std::min(jp_cdiv(total, TPB), 2048)), dim3(TPB), 0, st, labels, prev_labels, total);
    JP_LAUNCH_CHECK();
}
