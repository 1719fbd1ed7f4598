// Weight packing of the conv2d kernels: the pack kernels, the recorder of pack jobs and their one-launch replay.
//
// The MFMA kernels read their A operand (the weights) from a packed copy whose layout depends on the
// kernel family (the PACK_* modes of conv_pack.h, one case of pack_elem each).  A pack is a pure function of the weight
// tensor, so it only has to be redone when the weights change -- once per training step, after the optimizer.  Every
// pack goes through do_pack(), which
//   * launches it right away (ws_state 0 of the conv entry points: the caller's scratch holds nothing yet), and
//   * appends a 64-byte job descriptor to the caller's host buffer while a recording is open (jp_pack_record_begin).
// The host keeps the descriptors of all layers in one device table and refreshes EVERY pack of the model with ONE
// launch of jp_pack_replay per step (conv entry points then run with ws_state 1 = "scratch already packed"): ~310
// tiny launches per step become one.
#include "conv_pack.h"
#include "igemm_p9.h"       // P9_QAHEAD: slack quads of the PACK_FRAG layout
#include "igemm_p9s.h"      // JP_NS, JP_PACK_HDR, P9S_AHEAD, jp_split_ns: the split layouts
#include "scale.h"
#include <algorithm>

namespace {

struct JpPackJob {          // 64 bytes, mirrored by jperceiver_amd/ops.py (struct layout "PPqqi6i")
    const float* w;
    float* wp;
    long total, begin;      // elements of this pack; prefix offset inside a replay table
    int mode, p[6];
};
static_assert(sizeof(JpPackJob) == 64, "JpPackJob layout");
__host__ __device__ inline int jp_cdiv_d(int a, int b) { return (a + b - 1) / b; }

// taps a (class, slot) pair of the parity-class form stands for: dy in [y0, y1], dx in [x0, x1]
__device__ __forceinline__ float pack_slot_sum(const float* wc, int pl) {
    const int a = pl >> 3, b = (pl >> 2) & 1, r = (pl >> 1) & 1, sx = pl & 1;
    // Dy(a, r): a=0 -> {0} / {1,2};  a=1 -> {0,1} / {2}
    const int y0 = a ? (r ? 2 : 0) : (r ? 1 : 0), y1 = a ? (r ? 2 : 1) : (r ? 2 : 0);
    const int x0 = b ? (sx ? 2 : 0) : (sx ? 1 : 0), x1 = b ? (sx ? 2 : 1) : (sx ? 2 : 0);
    float v = 0.f;
    for (int dy = y0; dy <= y1; ++dy)
        for (int dx = x0; dx <= x1; ++dx) v += wc[dy * 3 + dx];
    return v;
}

__device__ __forceinline__ float pack_elem(int mode, const float* __restrict__ w, long i, const int* p, float sc = 1.f) {
    switch (mode) {
        case PACK_TAP: {       // p = Cout, Cin, KHW, Cp, for_dgrad: wp[tap][row][Cp], rows = Cout (fwd) / Cin (dgrad)
            const int Cout = p[0], Cin = p[1], KHW = p[2], Cp = p[3], for_dgrad = p[4];
            const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
            const int c = (int)(i % Cp);
            const long t = i / Cp;
            const int r = (int)(t % rows), tap = (int)(t / rows);
            if (c >= red) return 0.f;
            const int co = for_dgrad ? c : r, ci = for_dgrad ? r : c;
            return w[((size_t)co * Cin + ci) * KHW + tap];
        }
        case PACK_ROWMAJOR: {  // p = Cout, Cin, KHW, CP, Kp: wp[m][k = tap*CP + c] (zero padded to Kp), stem convs
            const int Cin = p[1], KHW = p[2], CP = p[3], Kp = p[4];
            const int k = (int)(i % Kp), m = (int)(i / Kp);
            const int tap = k / CP, c = k - tap * CP;
            return (tap < KHW && c < Cin) ? w[((size_t)m * Cin + c) * KHW + tap] : 0.f;
        }
        case PACK_SEG: {       // p = Cout, Cin, c_off, C, Cp, up: one channel segment [c_off, c_off + C); full resolution
                               // -> wp[tap][co][Cp]; upsampled -> wp[class][slot][co][Cp] (pre-summed taps)
            const int Cout = p[0], Cin = p[1], c_off = p[2], C = p[3], Cp = p[4], up = p[5];
            const int c = (int)(i % Cp);
            const long t = i / Cp;
            const int co = (int)(t % Cout), pl = (int)(t / Cout);
            if (c >= C) return 0.f;
            const float* wc = w + ((size_t)co * Cin + c_off + c) * 9;
            return up ? pack_slot_sum(wc, pl) : wc[pl];
        }
        case PACK_UP_DGRAD: {  // p = Cout, Cin, c_off, Cx, Cp: wpT[(class, slot)][c][co_pad] (dgrad A of the upsampled segment)
            const int Cout = p[0], Cin = p[1], c_off = p[2], Cx = p[3], Cp = p[4];
            const int co = (int)(i % Cp);
            const long t = i / Cp;
            const int c = (int)(t % Cx), pl = (int)(t / Cx);
            if (co >= Cout) return 0.f;
            return pack_slot_sum(w + ((size_t)co * Cin + c_off + c) * 9, pl);
        }
        case PACK_FRAG: {      // p = Cout, Cin, for_dgrad, BMT, KHW (9 or 1): MFMA fragment order of the P9 / P1 kernel (igemm_p9.h):
                               // wp[M tile][quad Q (+ slack quads)][k parity][row in tile][j] = W(row, reduction channel
                               // chunk*32 + 2s + parity, tap) for k-step 4Q + j = (chunk*KHW + tap)*16 + s: a lane's four
                               // k-steps of a quad are one 16-byte load; zero beyond the last step / row / channel
            const int Cout = p[0], Cin = p[1], for_dgrad = p[2], BMT = p[3], KHW = p[4];
            const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
            const long per_tile = ((long)((red + 31) / 32) * KHW * 4 + P9_QAHEAD + 1) * 8 * BMT;
            const int mt = (int)(i / per_tile);
            long t = i - (long)mt * per_tile;
            const int j = (int)(t & 3); t >>= 2;
            const int m = mt * BMT + (int)(t % BMT);
            t /= BMT;
            const int par = (int)(t & 1); t >>= 1;          // t = quad
            const long step = t * 4 + j;                    // global k-step
            const int s_ = (int)(step & 15);
            const long tc = step >> 4;                      // chunk*KHW + tap
            const int tap = (int)(tc % KHW);
            const int c = (int)(tc / KHW) * 32 + 2 * s_ + par;
            if (m >= rows || c >= red) return 0.f;
            const int co = for_dgrad ? c : m, ci = for_dgrad ? m : c;
            return w[((size_t)co * Cin + ci) * KHW + tap];
        }
        case PACK_SPLIT: {     // p = Cout, Cin, for_dgrad, BMT, KHW (9 or 1), KGS: split weights (JP_NS planes; i counts behind the pack header) in the fragment order
                               // of the P9S kernel (igemm_p9s.h): wp[M tile][step = (stage, tap, 16-channel group) (+ slack)]
                               // [split][k-half][row][4 words]; word w4 = the bf16 pair of reduction channels
                               // stage*16*KGS + group*16 + khalf*8 + 2*w4 + {0, 1} (low half = the even channel)
            const int Cout = p[0], Cin = p[1], for_dgrad = p[2], BMT = p[3], KHW = p[4], KGS = p[5];
            const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
            const long nsteps = (long)(red / (16 * KGS)) * KHW * KGS;
            const long per_tile = (nsteps + P9S_AHEAD) * (JP_NS * 8) * BMT;
            const int mt = (int)(i / per_tile);
            long t = i - (long)mt * per_tile;
            const int w4 = (int)(t & 3); t >>= 2;
            const int m = mt * BMT + (int)(t % BMT);
            t /= BMT;
            const int khalf = (int)(t & 1); t >>= 1;
            const int sp = (int)(t % JP_NS);
            const long U = t / JP_NS;
            if (U >= nsteps || m >= rows) return 0.f;
            const int stage = (int)(U / (KHW * KGS)), u = (int)(U % (KHW * KGS));
            const int tap = u / KGS, kg = u % KGS;
            const int c = stage * 16 * KGS + kg * 16 + khalf * 8 + 2 * w4;
            float v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int cc = c + k;
                const int co = for_dgrad ? cc : m, ci = for_dgrad ? m : cc;
                v[k] = cc < red ? w[((size_t)co * Cin + ci) * KHW + tap] : 0.f;
            }
            unsigned sq[3];
            jp_split_ns(v[0], v[1], sc, sq);
            return __uint_as_float(sp == 0 ? sq[0] : (sp == 1 ? sq[1] : sq[2]));
        }
        case PACK_SPLIT7: {    // p = Cout (<= 64), Cin: 7x7 stem weights as bf16 three-way splits in the fragment order of the P7S kernel
                               // (igemm_p7s.h): [step u = (c, tap-row pair v)][split][k-half][64 rows][4 words]; word w4 of k-half h =
                               // the taps (ky = 2v + h, kx = 2*w4 + {0, 1}) of channel c = u / 4 (ky, kx = 7: zero padding)
            const int Cout = p[0], Cin = p[1];
            const int w4 = (int)(i & 3), m = (int)((i >> 2) & 63), khalf = (int)((i >> 8) & 1);
            const long t = i >> 9;
            const int sp = (int)(t % JP_NS);
            const long U = t / JP_NS;
            const int c = (int)(U >> 2), ky = 2 * (int)(U & 3) + khalf;
            float v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int kx = 2 * w4 + k;
                v[k] = (c < Cin && m < Cout && ky < 7 && kx < 7) ? w[(((size_t)m * Cin + c) * 7 + ky) * 7 + kx] : 0.f;
            }
            unsigned sq[3];
            jp_split_ns(v[0], v[1], sc, sq);
            return __uint_as_float(sp == 0 ? sq[0] : (sp == 1 ? sq[1] : sq[2]));
        }
        case PACK_SPLITUPD: {  // p = Cout, Cin, c_off, Cx: dgrad weights of the upsampled iconv segment as bf16 three-way splits in the
                               // fragment order of the P9SD kernel (igemm_p9sd.h): [M tile of 128 rows c][step = (16-channel stage
                               // of co, (class, slot) q)][split][k-half][row][4 words]; value = the pre-summed slot weight W'_q[co][c]
            const int Cout = p[0], Cin = p[1], c_off = p[2], Cx = p[3];
            const long nsteps = (long)((Cout + 31) / 32 * 2) * 16;
            const long per_tile = (nsteps + P9S_AHEAD) * (JP_NS * 1024);
            const int mt = (int)(i / per_tile);
            long t = i - (long)mt * per_tile;
            const int w4 = (int)(t & 3); t >>= 2;
            const int c = mt * 128 + (int)(t & 127); t >>= 7;
            const int khalf = (int)(t & 1); t >>= 1;
            const int sp = (int)(t % JP_NS);
            const long U = t / JP_NS;
            if (U >= nsteps || c >= Cx) return 0.f;
            const int stage = (int)(U >> 4), q = (int)(U & 15);
            const int co = stage * 16 + khalf * 8 + 2 * w4;
            float v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k)
                v[k] = co + k < Cout ? pack_slot_sum(w + ((size_t)(co + k) * Cin + c_off + c) * 9, q) : 0.f;
            unsigned sq[3];
            jp_split_ns(v[0], v[1], sc, sq);
            return __uint_as_float(sp == 0 ? sq[0] : (sp == 1 ? sq[1] : sq[2]));
        }
        case PACK_SPLITSEG: {  // p = Cout, Cin, c_off, C, up, hdr_back: one channel segment of an iconv bank as JP_NS-way splits (the scale header
                               // of the bank sits hdr_back words in front of this segment, JP_NS == 2) in the
                               // fragment order of the P9US2 kernel (igemm_p9us2.h): [class (up only)][M tile of 128][step = (16-channel
                               // stage, tap | slot)][split][k-half][row 128][4 words]; word w4 = channels stage*16 + khalf*8 + 2*w4 + {0,1}
            const int Cout = p[0], Cin = p[1], c_off = p[2], C = p[3], up = p[4];
            const int T = up ? 4 : 9, MT = Cout / 128;
            const long tile = (long)((C + 15) / 16) * T * (JP_NS * 1024);
            const int cm = (int)(i / tile);
            if (cm >= (up ? 4 : 1) * MT) return 0.f;            // slack words behind the last stream
            long t = i - (long)cm * tile;
            const int cls = cm / MT, mt = cm - cls * MT;
            const int w4 = (int)(t & 3); t >>= 2;
            const int row = (int)(t & 127); t >>= 7;
            const int khalf = (int)(t & 1); t >>= 1;
            const int sp = (int)(t % JP_NS);
            const int U = (int)(t / JP_NS);
            const int stage = U / T, tap = U - stage * T;
            const int c = stage * 16 + khalf * 8 + 2 * w4, co = mt * 128 + row;
            float v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float* wc = w + ((size_t)co * Cin + c_off + c + k) * 9;
                v[k] = (c + k < C && co < Cout) ? (up ? pack_slot_sum(wc, cls * 4 + tap) : wc[tap]) : 0.f;
            }
            unsigned sq[3];
            jp_split_ns(v[0], v[1], sc, sq);
            return __uint_as_float(sp == 0 ? sq[0] : (sp == 1 ? sq[1] : sq[2]));
        }
        case PACK_FRAGSEG: {   // p = Cout, Cin, c_off, C, KP, up: one channel segment of an iconv bank in the fragment order of
                               // the P9U kernel (igemm_p9u.h): [class (up only)][M tile of 128][quad][k parity][row][4],
                               // k-step 4*quad + j = (stage, tap | slot, k-pair s) with 2*KP channels per stage
            const int Cout = p[0], Cin = p[1], c_off = p[2], C = p[3], KP = p[4], up = p[5];
            const int T = up ? 4 : 9, MT = Cout / 128;
            const long tile = (long)((C + 2 * KP - 1) / (2 * KP)) * T * KP / 4 * 1024;
            const int cm = (int)(i / tile);
            long t = i - (long)cm * tile;
            const int cls = cm / MT, mt = cm - cls * MT;
            const int j = (int)(t & 3); t >>= 2;
            const int row = (int)(t & 127); t >>= 7;
            const int par = (int)(t & 1); t >>= 1;          // t = quad
            const long step = t * 4 + j;
            const int stage = (int)(step / (T * KP)), rem = (int)(step - (long)stage * (T * KP));
            const int tap = rem / KP, s_ = rem - tap * KP;
            const int c = stage * 2 * KP + 2 * s_ + par, co = mt * 128 + row;
            if (c >= C || co >= Cout) return 0.f;
            const float* wc = w + ((size_t)co * Cin + c_off + c) * 9;
            return up ? pack_slot_sum(wc, cls * 4 + tap) : wc[tap];
        }
        default: {             // PACK_FLIP, p = Cout, Cin, c_off, C: wf[c][co][t] = w[co][c_off + c][8 - t]
            const int Cout = p[0], Cin = p[1], c_off = p[2];
            const int t = (int)(i % 9), co = (int)((i / 9) % Cout), c = (int)(i / (9 * (long)Cout));
            return w[((size_t)co * Cin + c_off + c) * 9 + 8 - t];
        }
    }
}

// Split packs of the fp16 two-way scheme (JP_NS == 2) start with a header {s, 1 / s, 0, 0}: s = the power of two that puts the weight
// tensor's largest magnitude into [2^14, 2^15) (jp_scale_exp); the fragments hold the splits of s * w.  pack_scale_kernel writes the
// headers (one workgroup per job) BEFORE the pack kernels of the same stream read them.
__device__ __forceinline__ int pack_hdr(int mode) { return (mode == PACK_SPLIT || mode == PACK_SPLITUPD || mode == PACK_SPLIT7) ? JP_PACK_HDR : 0; }
// the weight scale a split pack's elements are multiplied by: PACK_SPLIT's own header; PACK_SPLITSEG: the bank's header, p[5] words back
__device__ __forceinline__ float pack_scale_of(const JpPackJob& j) {
    if (!JP_PACK_HDR) return 1.f;
    if (j.mode == PACK_SPLIT || j.mode == PACK_SPLITUPD || j.mode == PACK_SPLIT7) return j.wp[0];
    if (j.mode == PACK_SPLITSEG) return *(j.wp - j.p[5]);
    return 1.f;
}
// Three small launches: zero the reduction word (header word 2) -- PSL workgroups per job reduce a slice of the weight tensor each into it
// (a maximum: order-independent) -- one thread per job turns it into {s, 1 / s}.  (One workgroup per job, as first written, took 2 ms per
// step on the 512 x 512 x 9 tensors: profiles/r05_fp16x2_first_kernel_stats.md.)
constexpr int PSL = 32;
__device__ __forceinline__ float* pack_scale_hdr(const JpPackJob& j, long* n) {
    const bool seg = j.mode == PACK_SPLITSEG && j.p[2] == 0;          // the bank's first segment owns the bank's header
    const bool upd = j.mode == PACK_SPLITUPD;                         // (pre-summed slot weights of the whole tensor: x 4 bound, like seg)
    const bool s7 = j.mode == PACK_SPLIT7;
    if (!JP_PACK_HDR || !(j.mode == PACK_SPLIT || seg || upd || s7)) return nullptr;
    *n = (long)j.p[0] * j.p[1] * ((seg || upd) ? 9 : (s7 ? 49 : j.p[4]));
    return seg ? j.wp - j.p[5] : j.wp;
}
__device__ __forceinline__ void pack_scale_zero(const JpPackJob& j) {
    long n;
    float* hdr = pack_scale_hdr(j, &n);
    if (hdr && threadIdx.x == 0) reinterpret_cast<unsigned*>(hdr)[2] = 0u;
}
__device__ __forceinline__ void pack_scale_reduce(const JpPackJob& j, int slice) {
    long n;
    float* hdr = pack_scale_hdr(j, &n);
    if (!hdr) return;
    const long per = (n + PSL - 1) / PSL, beg = slice * per, end = min(n, beg + per);
    unsigned m = 0;
    for (long i = beg + threadIdx.x; i < end; i += 256) m = max(m, jp_amag(__float_as_uint(j.w[i])));    // largest ordinary magnitude (scale.hip)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(reinterpret_cast<unsigned*>(hdr) + 2, m);
}
__device__ __forceinline__ void pack_scale_finish(const JpPackJob& j) {
    long n;
    float* hdr = pack_scale_hdr(j, &n);
    if (!hdr || threadIdx.x) return;
    // (iconv banks: the upsampled segment's elements are sums of up to four taps -- pack_slot_sum -- and all segments share one scale)
    const int k = jp_scale_exp(hdr[2] * ((j.mode == PACK_SPLITSEG || j.mode == PACK_SPLITUPD) ? 4.f : 1.f));
    hdr[0] = jp_exp2i(k);
    hdr[1] = jp_exp2i(-k);
    hdr[2] = hdr[3] = 0.f;
}
__global__ __launch_bounds__(64) void pack_scale_zero_one_kernel(JpPackJob job) { pack_scale_zero(job); }
__global__ __launch_bounds__(256) void pack_scale_reduce_one_kernel(JpPackJob job) { pack_scale_reduce(job, blockIdx.x); }
__global__ __launch_bounds__(64) void pack_scale_finish_one_kernel(JpPackJob job) { pack_scale_finish(job); }
__global__ __launch_bounds__(64) void pack_scale_zero_kernel(const JpPackJob* __restrict__ jobs, int njobs) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q < njobs) { long n; float* hdr = pack_scale_hdr(jobs[q], &n); if (hdr) reinterpret_cast<unsigned*>(hdr)[2] = 0u; }
}
__global__ __launch_bounds__(256) void pack_scale_reduce_kernel(const JpPackJob* __restrict__ jobs, int njobs) {
    pack_scale_reduce(jobs[blockIdx.y], blockIdx.x);
}
__global__ __launch_bounds__(64) void pack_scale_finish_kernel(const JpPackJob* __restrict__ jobs, int njobs) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q < njobs) {
        long n;
        float* hdr = pack_scale_hdr(jobs[q], &n);
        if (hdr) {
            const int k = jp_scale_exp(hdr[2] * ((jobs[q].mode == PACK_SPLITSEG || jobs[q].mode == PACK_SPLITUPD) ? 4.f : 1.f));
            hdr[0] = jp_exp2i(k);
            hdr[1] = jp_exp2i(-k);
            hdr[2] = hdr[3] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void pack_one_kernel(JpPackJob job) {
    const int hdr = pack_hdr(job.mode);
    const float sc = pack_scale_of(job);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < job.total - hdr; i += (long)gridDim.x * 256)
        job.wp[hdr + i] = pack_elem(job.mode, job.w, i, job.p, sc);
}

// every pack of the model in one launch.  The concatenated element range is walked in groups of FOUR consecutive elements
// (the host aligns every job's begin to a multiple of 4, jp_pack_replay contract): one binary search over the prefix
// offsets per group, and for the fragment-order packs -- most of the elements -- one index decode per group (the four
// elements are the four k-steps j of one quad: same tile, row, parity and tap) and one 16-byte store.
__global__ __launch_bounds__(256) void pack_replay_kernel(const JpPackJob* __restrict__ jobs, int njobs, long total) {
    const long groups = (total + 3) >> 2;
    for (long g4 = (long)blockIdx.x * 256 + threadIdx.x; g4 < groups; g4 += (long)gridDim.x * 256) {
        const long g = g4 << 2;
        int lo = 0, hi = njobs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].begin <= g) lo = mid; else hi = mid - 1;
        }
        const JpPackJob& j = jobs[lo];
        const long i = g - j.begin;
        if (i >= j.total) continue;                         // alignment padding between two jobs
        if (j.mode == PACK_SPLIT || j.mode == PACK_SPLITSEG) continue;      // pack_split_replay_kernel's
        if (j.mode == PACK_FRAG && i + 4 <= j.total) {
            const int* p = j.p;
            const int Cout = p[0], Cin = p[1], for_dgrad = p[2], BMT = p[3], KHW = p[4];
            const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
            const long per_tile = ((long)((red + 31) / 32) * KHW * 4 + P9_QAHEAD + 1) * 8 * BMT;
            const int mt = (int)(i / per_tile);
            long t = (i - (long)mt * per_tile) >> 2;
            const int m = mt * BMT + (int)(t % BMT);
            t /= BMT;
            const int par = (int)(t & 1); t >>= 1;          // t = quad
            const long step = t * 4;                        // k-steps step .. step+3 share (chunk, tap)
            const int s0 = (int)(step & 15);
            const long tc = step >> 4;
            const int tap = (int)(tc % KHW), c0 = (int)(tc / KHW) * 32 + 2 * s0 + par;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < rows) {
                const size_t cs = for_dgrad ? (size_t)Cin * KHW : (size_t)KHW;      // stride of the reduction channel in w
                const float* wb = j.w + (for_dgrad ? (size_t)m * KHW : (size_t)m * Cin * KHW) + tap;
                if (c0 < red) v.x = wb[(size_t)c0 * cs];
                if (c0 + 2 < red) v.y = wb[(size_t)(c0 + 2) * cs];
                if (c0 + 4 < red) v.z = wb[(size_t)(c0 + 4) * cs];
                if (c0 + 6 < red) v.w = wb[(size_t)(c0 + 6) * cs];
            }
            *reinterpret_cast<float4*>(j.wp + i) = v;
        } else {
            // (split packs with a scale header -- PACK_SPLITUPD, PACK_SPLIT7: the header words belong to the pack_scale kernels, the
            // elements count from behind it and are the splits of scale * w)
            const int hdr = pack_hdr(j.mode);
            const float sc = hdr ? pack_scale_of(j) : 1.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k >= hdr && i + k < j.total) j.wp[i + k] = pack_elem(j.mode, j.w, i + k - hdr, j.p, sc);
        }
    }
}

// The split packs (PACK_SPLIT / PACK_SPLITSEG, most of the replayed bytes since round 3) through LDS: a work item = (job, M tile,
// 16*KGS-channel stage, chunk of 64 rows).  Its weights -- 64 rows x CS channels x KHW taps, contiguous runs of the weight tensor in
// either orientation -- are read COALESCED into LDS, then every (step, k-half, row) triple is split once and written as three
// 16-byte words; the 64 rows of a (step, split, k-half) are one contiguous 1 KB run of the pack.  (The generic replay decoded
// every 4-byte word on its own and read its two weights with a KHW-float stride: 1.3 ms per step at the head of the step.)
__device__ __forceinline__ int split_job_items(const JpPackJob& j) {
    const int* p = j.p;
    if (j.mode == PACK_SPLIT) {
        const int rows = p[2] ? p[1] : p[0], red = p[2] ? p[0] : p[1];
        return jp_cdiv_d(rows, p[3]) * (red / (16 * p[5])) * (p[3] / 64);
    }
    if (j.mode == PACK_SPLITSEG) return (p[0] / 128) * ((p[3] + 15) / 16) * 2;
    return 0;
}
__global__ __launch_bounds__(256) void pack_split_replay_kernel(const JpPackJob* __restrict__ jobs, int njobs) {
    __shared__ float tile[64 * 16 * 9 + 64];           // [row][channel][tap] (PACK_SPLIT fwd / SEG) or [channel][row][tap] (dgrad)
    constexpr int MAXJ = 2048;
    __shared__ int pre[MAXJ + 1];                       // exclusive prefix of the jobs' work-item counts
    const int t = threadIdx.x;
    for (int q = t; q < njobs && q < MAXJ; q += 256) pre[q + 1] = split_job_items(jobs[q]);
    if (t == 0) pre[0] = 0;
    __syncthreads();
    if (t == 0)
        for (int q = 1; q <= njobs && q <= MAXJ; ++q) pre[q] += pre[q - 1];
    __syncthreads();
    const int nj = min(njobs, MAXJ), total_items = pre[nj];
    for (int item = blockIdx.x; item < total_items; item += gridDim.x) {
        __syncthreads();                                // the tile of the previous item is no longer read
        int lo = 0, hi = nj - 1;                        // last job whose prefix <= item
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const int jj = lo, loc = item - pre[lo];
        const JpPackJob& j = jobs[jj];
        const int* p = j.p;
        unsigned* out = reinterpret_cast<unsigned*>(j.wp) + pack_hdr(j.mode);
        if (j.mode == PACK_SPLIT) {
            const float wsc = JP_PACK_HDR ? j.wp[0] : 1.f;
            const int Cout = p[0], Cin = p[1], for_dgrad = p[2], BMT = p[3], KHW = p[4], KGS = p[5];
            const int rows = for_dgrad ? Cin : Cout, red = for_dgrad ? Cout : Cin;
            const int CS = 16 * KGS, nst = red / CS, rch = BMT / 64;
            const int rc = loc % rch, stage = (loc / rch) % nst, mt = loc / (rch * nst);
            const int m0 = mt * BMT + rc * 64, c0 = stage * CS;
            const int RUN = CS * KHW;                   // floats of one row (fwd) -- or 64*KHW of one channel (dgrad)
            if (!for_dgrad) {
                for (int e = t; e < 64 * RUN; e += 256) {
                    const int r = e / RUN, o = e - r * RUN;
                    tile[e] = (m0 + r < rows) ? j.w[((size_t)(m0 + r) * Cin + c0) * KHW + o] : 0.f;
                }
            } else {
                const int RUNd = 64 * KHW;
                for (int e = t; e < CS * RUNd; e += 256) {
                    const int c = e / RUNd, o = e - c * RUNd;            // o = r*KHW + tap
                    tile[e] = (m0 + o / KHW < rows) ? j.w[((size_t)(c0 + c) * Cin + m0) * KHW + o] : 0.f;
                }
            }
            __syncthreads();
            const long nsteps = (long)nst * KHW * KGS;
            const long per_tile = (nsteps + P9S_AHEAD) * (JP_NS * 8) * BMT;
            const int trip = KHW * KGS * 2 * 64;        // (tap, group, k-half, row) triples of this item
            for (int e = t; e < trip; e += 256) {
                const int r = e & 63, kh = (e >> 6) & 1, u = e >> 7;      // u = tap*KGS + kg
                const int tap = u / KGS, kg = u - tap * KGS;
                jp_u32x4 w0, w1, w2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = kg * 16 + kh * 8 + 2 * k;
                    const float a = for_dgrad ? tile[(c * 64 + r) * KHW + tap] : tile[(r * CS + c) * KHW + tap];
                    const float b = for_dgrad ? tile[((c + 1) * 64 + r) * KHW + tap] : tile[(r * CS + c + 1) * KHW + tap];
                    unsigned sq[3];
                    jp_split_ns(a, b, wsc, sq);
                    w0[k] = sq[0]; w1[k] = sq[1]; w2[k] = sq[2];
                }
                const long U = (long)stage * KHW * KGS + u;
                unsigned* q = out + (long)mt * per_tile + ((U * JP_NS) * 2 + kh) * (long)BMT * 4 + (long)(rc * 64 + r) * 4;
                *reinterpret_cast<jp_u32x4*>(q) = w0;
                *reinterpret_cast<jp_u32x4*>(q + 2L * BMT * 4) = w1;
                if (JP_NS == 3) *reinterpret_cast<jp_u32x4*>(q + 4L * BMT * 4) = w2;
            }
        } else {            // PACK_SPLITSEG: p = Cout, Cin, c_off, C, up
            const int Cout = p[0], Cin = p[1], c_off = p[2], C = p[3], up = p[4];
            const int T = up ? 4 : 9, MT = Cout / 128, nst = (C + 15) / 16;
            const int rc = loc & 1, stage = (loc >> 1) % nst, mt = (loc >> 1) / nst;
            const int m0 = mt * 128 + rc * 64, c0 = stage * 16;
            for (int e = t; e < 64 * 144; e += 256) {
                const int r = e / 144, o = e - r * 144, c = o / 9;
                tile[e] = (c0 + c < C && m0 + r < Cout) ? j.w[((size_t)(m0 + r) * Cin + c_off + c0) * 9 + o] : 0.f;
            }
            __syncthreads();
            const long tl = (long)nst * T * (JP_NS * 1024);
            const int ncls = up ? 4 : 1, trip = ncls * T * 2 * 64;
            const float wsc = pack_scale_of(j);
            for (int e = t; e < trip; e += 256) {
                const int r = e & 63, kh = (e >> 6) & 1, ct = e >> 7, tap = ct % T, cls = ct / T;
                jp_u32x4 w0, w1, w2;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = kh * 8 + 2 * k;
                    const float* wa = tile + (r * 16 + c) * 9;
                    const float a = up ? pack_slot_sum(wa, cls * 4 + tap) : wa[tap];
                    const float b = up ? pack_slot_sum(wa + 9, cls * 4 + tap) : wa[9 + tap];
                    unsigned sq[3];
                    jp_split_ns(a, b, wsc, sq);
                    w0[k] = sq[0]; w1[k] = sq[1]; w2[k] = sq[2];
                }
                const long U = (long)stage * T + tap;
                unsigned* q = out + (long)(cls * MT + mt) * tl + ((U * JP_NS) * 2 + kh) * 512L + (long)(rc * 64 + r) * 4;
                *reinterpret_cast<jp_u32x4*>(q) = w0;
                *reinterpret_cast<jp_u32x4*>(q + 1024) = w1;
                if (JP_NS == 3) *reinterpret_cast<jp_u32x4*>(q + 2048) = w2;
            }
        }
    }
}

thread_local JpPackJob* g_pack_rec = nullptr;
thread_local int g_pack_rec_n = 0, g_pack_rec_cap = 0;

}  // namespace

void do_pack(int mode, const float* w, float* wp, long total, int p0, int p1, int p2, int p3, int p4, int p5, hipStream_t st) {
    JpPackJob j{w, wp, total, 0, mode, {p0, p1, p2, p3, p4, p5}};
    if (g_pack_rec) {
        if (g_pack_rec_n < g_pack_rec_cap) g_pack_rec[g_pack_rec_n] = j;
        ++g_pack_rec_n;      // counted even when the buffer is full: jp_pack_record_end reports the overflow
    }
    if (JP_PACK_HDR && (mode == PACK_SPLIT || mode == PACK_SPLITUPD || mode == PACK_SPLIT7 || (mode == PACK_SPLITSEG && p2 == 0))) {
        hipLaunchKernelGGL(pack_scale_zero_one_kernel, dim3(1), dim3(64), 0, st, j);
        hipLaunchKernelGGL(pack_scale_reduce_one_kernel, dim3(PSL), dim3(256), 0, st, j);
        hipLaunchKernelGGL(pack_scale_finish_one_kernel, dim3(1), dim3(64), 0, st, j);
    }
    hipLaunchKernelGGL(pack_one_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, j);
}

void pack_weights(const float* w, float* wp, int Cout, int Cin, int KHW, int Cp, int for_dgrad, hipStream_t st) {
    do_pack(PACK_TAP, w, wp, (long)KHW * (for_dgrad ? Cin : Cout) * Cp, Cout, Cin, KHW, Cp, for_dgrad, 0, st);
}

// ---- weight-pack recording / replay (see do_pack).  `host_jobs`: caller-owned HOST buffer of max_jobs 64-byte records.
extern "C" int jp_pack_job_bytes(void) { return (int)sizeof(JpPackJob); }

extern "C" int jp_pack_record_begin(void* host_jobs, int max_jobs) {
    JP_CHECK_ARG(host_jobs && max_jobs > 0 && !g_pack_rec, "pack_record_begin: bad args or a recording is already open");
    g_pack_rec = (JpPackJob*)host_jobs;
    g_pack_rec_n = 0;
    g_pack_rec_cap = max_jobs;
    return JP_OK;
}

// -> number of packs the conv entry points issued on this thread since jp_pack_record_begin (> max_jobs: overflow)
extern "C" int jp_pack_record_end(void) {
    g_pack_rec = nullptr;
    return g_pack_rec_n;
}

// jobs: DEVICE copy of `njobs` records whose `begin` fields hold the exclusive prefix sum of `total`; total_elems = the sum.
// 1 if a recorded job of this mode is re-packed by the LDS-staged split-pack kernel (its elements are skipped by the generic kernel):
// a caller that puts those jobs BEHIND the others in the table can tell jp_pack_replay where the generic kernel's range ends
extern "C" int jp_pack_mode_is_split(int mode) { return (mode == PACK_SPLIT || mode == PACK_SPLITSEG) ? 1 : 0; }
// generic_elems: elements (begin of the first split-pack job) the generic kernel has to walk when the split-pack jobs are the tail of
// the table; <= 0 or >= total_elems: the whole range (round 6: the generic kernel spent most of its 0.36 ms at the head of every step
// deciding, four elements at a time, that a range belongs to the other kernel)
extern "C" int jp_pack_replay(const void* jobs, int njobs, long total_elems, long generic_elems, void* stream) {
    JP_CHECK_ARG(jobs && njobs > 0 && total_elems > 0, "pack_replay: bad args");
    const long gen = (generic_elems > 0 && generic_elems < total_elems) ? generic_elems : total_elems;
    if (JP_PACK_HDR)    // headers (weight scales) of the fp16 split packs first: the pack kernels below read them
    {
        hipLaunchKernelGGL(pack_scale_zero_kernel, dim3((njobs + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const JpPackJob*)jobs, njobs);
        hipLaunchKernelGGL(pack_scale_reduce_kernel, dim3(PSL, njobs), dim3(256), 0, (hipStream_t)stream, (const JpPackJob*)jobs, njobs);
        hipLaunchKernelGGL(pack_scale_finish_kernel, dim3((njobs + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const JpPackJob*)jobs, njobs);
    }
    hipLaunchKernelGGL(pack_replay_kernel, dim3((int)std::min<long>((gen + 4095) / 4096, 16384)), dim3(256), 0,
                       (hipStream_t)stream, (const JpPackJob*)jobs, njobs, gen);
    // the split-bf16 packs of the table: LDS-staged, grid-stride over their work items (a block without an item returns)
    // (its job-prefix table lives in LDS: 2048 jobs per launch -- a model has a few hundred; longer tables go in slices)
    for (int off = 0; off < njobs; off += 2048)
        hipLaunchKernelGGL(pack_split_replay_kernel, dim3(4096), dim3(256), 0, (hipStream_t)stream, (const JpPackJob*)jobs + off,
                           std::min(2048, njobs - off));
    JP_LAUNCH_CHECK();
}
