// BEV object instances (apis/bevobj.py BevObjects; PerceptionStream(objects=...)): the connected components of one class of the layout
// (jp_layout_classes_u8; default 2 = car), numbered in raster order of their first cell, with one row of integer statistics each.  The
// library keeps no state: layout, grid, labels, count, table and the scratch are the caller's buffers, and everything the call leaves is
// overwritten by it (nothing to zero first).  One call enqueues FIVE launches with fixed arguments; a phase that needs a global order is
// a launch of its own: no workgroup waits on another (no grid barrier, no flag, no cooperative launch).
//   init    : one thread per cell.  A foreground cell points at the first cell of its horizontal run inside its wave's 64 cells (two
//             ballots, no memory traffic between cells); background cells get -1; the size words are zeroed.  Stores only.
//   unite   : the links that init left out, by lock-free atomicMin unions in global memory: a run that continues across a wave border
//             (lane 0 with its W neighbour), N unless W and NW are both foreground (then W's run carries the link), and under
//             8-connectivity NW unless N or W is foreground, NE unless N is.  unite() finds both roots, atomicMin's the larger root's
//             word with the smaller and follows the returned value when it differs: every trip lowers one of the two indices, so the
//             loop ends whatever other workgroups do.  The root of a component is its minimum index = its first cell in raster order,
//             whatever the order of arrival.
//   flatten : every cell walks to its root, stores it, and adds to the root's size word (one atomicAdd per distinct root of a wave).
//   number  : one workgroup per camera.  flag = root with size >= min_cells; exclusive prefix sum of the flags in raster order (every
//             wave owns a contiguous span: count, one LDS fold of 16 totals, number; the span is read 16 cells per lane at a time and
//             the flags of the first sweep stay in registers) -> the id at the root, -1 at a dropped root; count[b]; the camera's
//             table rows are set to the neutral element of the sums below (kept rows) or zero (the rest).
//   emit    : labels = id of the cell's root; every run of equal ids in a wave's row piece is folded by a segmented scan, the runs of
//             a workgroup's 1024 cells are folded per object in LDS, and the workgroup issues integer atomicAdd / atomicMin /
//             atomicMax / atomicOr on the object's row -- order-free, two runs give the same bytes.
// Indices are GLOBAL (b occ occ + i occ + j < 2^31): cameras share the launches and never share a component.
// Not built: an LDS strip phase -- the wave-local runs already remove the horizontal unions, what is left are the vertical
// ones, whose number an LDS strip of h rows would cut by h at the price of a second union-find in LDS.
#include "jp_common.h"
#include <climits>

namespace {
constexpr int TPB = 256;                                               // a multiple of 64: init and unite agree on the lanes
constexpr int NTPB = 1024, NW = NTPB / 64;
constexpr int NF = 12;                                                 // words of a table row
constexpr int NCH = 16, KEPT = 4;                                      // the numbering kernel: cells per lane in a chunk, chunks kept
constexpr int ETPB = 1024, SLOTS = 128;                                // the emit kernel: cells per workgroup, LDS rows (a power of two)
typedef unsigned long long u64;

// [cells, r_min, r_max, c_min, c_max, sum_r, sum_c, first_cell, edge_mask, pts, pts_obst, hmax_mm]: the neutral element of word f
__device__ __forceinline__ constexpr int neutral_of(int f) {
    return (f == 1 || f == 3) ? INT_MAX : ((f == 2 || f == 4 || f == 11) ? INT_MIN : 0);
}

// unite runs next to other workgroups' atomics on the same words: its loads must not be served from this CU's L1
__device__ __forceinline__ int live(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int find_live(const int* parent, int x) {
    for (int y; (y = live(parent + x)) != x;) x = y;                   // parent[x] <= x: strictly downhill
    return x;
}

__device__ void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_live(parent, a);
        b = find_live(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);                      // a > b
        if (old == a) return;                                          // a was still a root: it now hangs under b
        a = old;                                                       // somebody moved a first (old < a): (old, b) is what is left to join
    }
}

// first lane of the run that `lane` closes: the highest head at or below it
__device__ __forceinline__ int run_start(u64 heads, int lane) { return 63 - __clzll((long long)(heads & (~0ULL >> (63 - lane)))); }

__global__ __launch_bounds__(TPB) void bevobj_init_kernel(const uint8_t* __restrict__ layout, int* __restrict__ parent,
                                                          int* __restrict__ aux, int total, int occ, int cls) {
    const long gl = (long)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = gl < total;                                        // no thread leaves before the ballots
    const int g = in ? (int)gl : 0;
    const bool fg = in && layout[g] == cls;
    const int col = g % occ;                                           // column 0 also begins every camera
    const u64 mask = __ballot(fg);
    const bool head = fg && (lane == 0 || col == 0 || !((mask >> (lane - 1)) & 1ULL));
    const u64 heads = __ballot(head);
    if (!in) return;
    parent[g] = fg ? g - (lane - run_start(heads, lane)) : -1;
    aux[g] = 0;
}

__global__ __launch_bounds__(TPB) void bevobj_unite_kernel(const uint8_t* __restrict__ layout, int* parent, int total, int occ, int cells,
                                                           int cls, int conn8) {
    const long gl = (long)blockIdx.x * TPB + threadIdx.x;
    if (gl >= total) return;
    const int g = (int)gl, lane = threadIdx.x & 63;
    const uint8_t* l = layout + g;
    if (l[0] != cls) return;
    const int k = g % cells, row = k / occ, col = k - row * occ;
    const bool w = col > 0 && l[-1] == cls;
    const bool n = row > 0 && l[-occ] == cls;
    const bool nw = row > 0 && col > 0 && l[-occ - 1] == cls;
    if (w && lane == 0) unite(parent, g, g - 1);
    if (n && !(w && nw)) unite(parent, g, g - occ);
    if (conn8) {
        if (nw && !n && !w) unite(parent, g, g - occ - 1);
        if (!n && row > 0 && col < occ - 1 && l[-occ + 1] == cls) unite(parent, g, g - occ + 1);
    }
}

__global__ __launch_bounds__(TPB) void bevobj_flatten_kernel(int* parent, int* aux, int total) {
    const long gl = (long)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r = -1;
    if (gl < total && parent[gl] >= 0) {
        // other threads store roots into the words this walk reads: an old word and a new one both lead to the root
        r = (int)gl;
        for (int y; (y = parent[r]) != r;) r = y;
        parent[gl] = r;
    }
    u64 todo = __ballot(r >= 0);                                       // uniform: every lane stays to the end
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int root = __shfl(r, first, 64);
        const u64 same = __ballot(r == root);
        if (lane == first) atomicAdd(aux + root, __popcll(same));
        todo &= ~same;
    }
}

// The flags of one chunk of a wave's span: bit j of `root` / `keep` belongs to cell k0 + 64 j + lane (lanes run along the cells).
// All NCH loads of a lane are independent and issued together: the kernel below is one workgroup per camera, its time is the number
// of load latencies it waits for one after another.
__device__ __forceinline__ void chunk_flags(const int* parent, const int* aux, int base, int k0, int hi, int lane, int min_cells,
                                            unsigned& root, unsigned& keep) {
    int p[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int k = k0 + 64 * j + lane;
        p[j] = k < hi ? parent[base + k] : -1;
    }
    root = 0u;
#pragma unroll
    for (int j = 0; j < NCH; ++j) root |= (p[j] == base + k0 + 64 * j + lane ? 1u : 0u) << j;
#pragma unroll
    for (int j = 0; j < NCH; ++j) p[j] = (root >> j) & 1u ? aux[base + k0 + 64 * j + lane] : 0;       // sizes: at roots only
    keep = 0u;
#pragma unroll
    for (int j = 0; j < NCH; ++j) keep |= (((root >> j) & 1u) && p[j] >= min_cells ? 1u : 0u) << j;
}

// ids of a chunk's kept roots, in raster order (j, then the lane), from `run` on; -1 at its dropped roots.  -> the next id
__device__ __forceinline__ int number_chunk(int* aux, int g0, int lane, unsigned root, unsigned keep, int run) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const bool kp = (keep >> j) & 1u;
        const u64 m = __ballot(kp);
        if ((root >> j) & 1u) aux[g0 + 64 * j + lane] = kp ? run + __popcll(m & ((1ULL << lane) - 1ULL)) : -1;
        run += __popcll(m);
    }
    return run;
}

// grid (B).  aux: the size at every root on entry; the id (or -1: dropped) at every root on exit.
__global__ __launch_bounds__(NTPB) void bevobj_number_kernel(const int* parent, int* aux, int* __restrict__ count, int* __restrict__ table,
                                                             int cells, int min_cells, int max_objects) {
    __shared__ int wtot[NW];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int base = b * cells;
    constexpr int CH = 64 * NCH;                                       // cells of a chunk
    const int span = ((cells + NW * CH - 1) / (NW * CH)) * CH;         // cells per wave, whole chunks: NW spans cover the camera
    const int lo = w * span, hi = min(cells, lo + span);
    // the flags of the first KEPT chunks of the span stay in registers for the second sweep (occ <= 256: all of them)
    unsigned rootc[KEPT], keepc[KEPT];
    int n = 0;
#pragma unroll
    for (int c = 0; c < KEPT; ++c) {
        rootc[c] = keepc[c] = 0u;
        if (lo + c * CH < hi) chunk_flags(parent, aux, base, lo + c * CH, hi, lane, min_cells, rootc[c], keepc[c]);
        n += __popc(keepc[c]);
    }
    for (int k0 = lo + KEPT * CH; k0 < hi; k0 += CH) {
        unsigned root, keep;
        chunk_flags(parent, aux, base, k0, hi, lane, min_cells, root, keep);
        n += __popc(keep);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wtot[w] = n;
    __syncthreads();
    int run = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        run += i < w ? wtot[i] : 0;
        all += wtot[i];
    }
    // uniform trips: the ballots see the whole wave
#pragma unroll
    for (int c = 0; c < KEPT; ++c)
        if (lo + c * CH < hi) run = number_chunk(aux, base + lo + c * CH, lane, rootc[c], keepc[c], run);
    for (int k0 = lo + KEPT * CH; k0 < hi; k0 += CH) {
        unsigned root, keep;
        chunk_flags(parent, aux, base, k0, hi, lane, min_cells, root, keep);
        run = number_chunk(aux, base + k0, lane, root, keep, run);
    }
    if (threadIdx.x == 0) count[b] = all;
    int* rows = table + (long)b * max_objects * NF;
    const int kept = min(all, max_objects);
    for (int i = threadIdx.x; i < max_objects * NF; i += NTPB) {
        const int row = i / NF, f = i - row * NF;
        rows[i] = row < kept ? neutral_of(f) : 0;
    }
}

// one value of a run (or of a workgroup's slot) into word f of a table row
__device__ __forceinline__ void fold(int* word, int f, int v) {
    if (v == neutral_of(f)) return;
    if (f == 1 || f == 3) atomicMin(word, v);
    else if (f == 2 || f == 4 || f == 11) atomicMax(word, v);
    else if (f == 8) atomicOr(word, v);
    else atomicAdd(word, v);
}

// A workgroup of ETPB consecutive cells.  Most of a large object's runs meet others of the same object in their workgroup: they are
// folded in LDS first (SLOTS direct-mapped rows, claimed by compare-and-swap; a run whose slot is taken by another object goes to
// global memory itself) and the workgroup then issues one set of global atomics per object it holds -- same-address global atomics
// are what this kernel's time is made of (profiles/bev_objects.md).
__global__ __launch_bounds__(ETPB) void bevobj_emit_kernel(const int* __restrict__ parent, const int* __restrict__ aux,
                                                           const int* __restrict__ grid, int* __restrict__ labels, int* table, int total,
                                                           int occ, int cells, int max_objects) {
    __shared__ int tag[SLOTS];
    __shared__ int acc[SLOTS][NF];
    for (int i = threadIdx.x; i < SLOTS * NF; i += ETPB) acc[i / NF][i % NF] = neutral_of(i % NF);
    if (threadIdx.x < SLOTS) tag[threadIdx.x] = -1;
    __syncthreads();
    const long gl = (long)blockIdx.x * ETPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int id = -1, b = 0, k = 0, row = 0, col = 0;
    bool first = false;
    if (gl < total) {
        const int g = (int)gl, r = parent[g];
        b = g / cells;
        k = g - b * cells;
        row = k / occ;
        col = k - row * occ;
        if (r >= 0) id = aux[r];
        first = r == g;
        labels[g] = id;
    }
    const int tid = id < max_objects ? id : -1;                         // the object's table row, -1: none (background, dropped, overflow)
    int n = tid >= 0 ? 1 : 0, sc = col, pts = 0, po = 0, hm = INT_MIN;
    if (tid >= 0 && grid) {
        const int* gp = grid + (long)b * 4 * cells + k;
        pts = gp[0];
        po = gp[cells];
        if (pts > 0) hm = gp[3L * cells];
    }
    const int trow = b * max_objects + (tid >= 0 ? tid : 0);            // row of the whole table: B max_objects 12 < 2^31
    int* t = table + (long)trow * NF;
    if (tid >= 0 && first) t[7] = k;                                    // the root is the first cell: one lane per object stores it
    // a run = consecutive lanes of one image row with one id (column 0 begins a row and a camera)
    const int before = __shfl_up(tid, 1, 64);
    const bool head = lane == 0 || col == 0 || before != tid;
    const u64 heads = __ballot(head);
    const int start = run_start(heads, lane);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                                  // inclusive scan over [start, lane]
        const int n2 = __shfl_up(n, o, 64), sc2 = __shfl_up(sc, o, 64), pts2 = __shfl_up(pts, o, 64), po2 = __shfl_up(po, o, 64),
                  hm2 = __shfl_up(hm, o, 64);
        if (lane - o >= start) {
            n += n2;
            sc += sc2;
            pts += pts2;
            po += po2;
            hm = max(hm, hm2);
        }
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ULL);
    if (tid >= 0 && tail) {
        const int c0 = col - n + 1;
        const int edge = (row == 0 ? 1 : 0) | (row == occ - 1 ? 2 : 0) | (c0 == 0 ? 4 : 0) | (col == occ - 1 ? 8 : 0);
        const int v[NF] = {n, row, row, c0, col, n * row, sc, 0, edge, pts, po, hm};
        const int slot = trow & (SLOTS - 1);
        const int owner = atomicCAS(&tag[slot], -1, trow);
        if (owner == -1 || owner == trow) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
                if (f != 7) fold(&acc[slot][f], f, v[f]);
        } else {
#pragma unroll
            for (int f = 0; f < NF; ++f)
                if (f != 7) fold(t + f, f, v[f]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS * NF; i += ETPB) {
        const int slot = i / NF, f = i - slot * NF, owner = tag[slot];
        if (owner >= 0 && f != 7) fold(table + (long)owner * NF + f, f, acc[slot][f]);
    }
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" long jp_bev_objects_ws_bytes(int B, int occ) {
    if (B <= 0 || occ <= 0) return 0;
    return 2L * sizeof(int) * B * occ * occ;                           // parent, aux: one word per cell each
}

extern "C" int jp_bev_objects(const uint8_t* layout, const int* grid, int* labels, int* count, int* table, void* ws, int B, int occ,
                              int cls_value, int conn, int min_cells, int max_objects, void* stream) {
    JP_CHECK_ARG(layout && labels && count && table && ws, "bev_objects: null pointer (layout, labels, count, table and ws are required)");
    JP_CHECK_ARG(B > 0 && occ > 0 && max_objects > 0, "bev_objects: B, occ and max_objects must be positive");
    JP_CHECK_ARG(min_cells >= 1, "bev_objects: min_cells must be at least 1");
    JP_CHECK_ARG(conn == 4 || conn == 8, "bev_objects: conn must be 4 or 8");
    JP_CHECK_ARG(cls_value >= 0 && cls_value <= 255, "bev_objects: cls_value must lie in 0 .. 255 (the layout holds bytes)");
    JP_CHECK_ARG(occ <= 1024, "bev_objects: occ must not exceed 1024 (sum_r is an int32: 1024^2 * 1023 < 2^31)");
    JP_CHECK_ARG((long)B * max_objects * NF < (1L << 31), "bev_objects: B * max_objects * 12 must be below 2^31");
    JP_CHECK_ARG((long)B * occ * occ < (1L << 31), "bev_objects: B * occ * occ must be below 2^31");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int cells = occ * occ, total = B * cells;
    int* parent = static_cast<int*>(ws);
    int* aux = parent + total;
    const dim3 blocks(jp_cdiv(total, TPB));
    hipLaunchKernelGGL(bevobj_init_kernel, blocks, dim3(TPB), 0, st, layout, parent, aux, total, occ, cls_value);
    hipLaunchKernelGGL(bevobj_unite_kernel, blocks, dim3(TPB), 0, st, layout, parent, total, occ, cells, cls_value, conn == 8 ? 1 : 0);
    hipLaunchKernelGGL(bevobj_flatten_kernel, blocks, dim3(TPB), 0, st, parent, aux, total);
    hipLaunchKernelGGL(bevobj_number_kernel, dim3(B), dim3(NTPB), 0, st, parent, aux, count, table, cells, min_cells, max_objects);
    hipLaunchKernelGGL(bevobj_emit_kernel, dim3(jp_cdiv(total, ETPB)), dim3(ETPB), 0, st, parent, aux, grid, labels, table, total, occ,
                       cells, max_objects);
    JP_LAUNCH_CHECK();
}
