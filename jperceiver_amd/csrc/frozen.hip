// Frozen inference (model/modules.py FrozenConvBN, apis.freeze): an eval-mode BatchNorm2d behind a convolution is a fixed per-channel
// affine map, so it is folded into the convolution's weights and bias ONCE (jp_bn_fold_conv) and the convolution's own bias / activation
// epilogue does the rest.  What is left of `conv -> BN -> (+residual) -> ReLU` at the end of a BasicBlock (resnet.py:41-45) is one
// element-wise pass, jp_add_relu -- the only kernel of the feature that runs per frame.
#include "jp_common.h"
#include <algorithm>
#include <cstdint>

namespace {
constexpr int TPB = 256;

// One workgroup per output channel.  s = gamma / sqrt(var + eps) and the folded bias in float64, every product rounded to float once.
// The explicit round-to-nearest intrinsics keep -ffp-contract from fusing (b - mean) * s + beta into an fma: the result is the formula
// as written, operation by operation (negative, zero and tiny gamma included: nothing is clamped).
__global__ __launch_bounds__(TPB) void bn_fold_conv_kernel(const float* __restrict__ w, const float* __restrict__ cb,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                                           float* __restrict__ w_out, float* __restrict__ b_out, int K) {
    const int c = blockIdx.x;
    const double s = (double)gamma[c] / sqrt(__dadd_rn((double)rv[c], (double)eps));
    const float* wr = w + (size_t)c * K;
    float* wo = w_out + (size_t)c * K;
    for (int k = threadIdx.x; k < K; k += TPB) wo[k] = (float)__dmul_rn((double)wr[k], s);
    if (threadIdx.x == 0) {
        const double b = cb ? (double)cb[c] : 0.0;
        b_out[c] = (float)__dadd_rn((double)beta[c], __dmul_rn(__dadd_rn(b, -(double)rm[c]), s));
    }
}

// out = a + b, then max(., 0): 16 bytes per lane and access while all three pointers sit on a 16-byte boundary (n4 = n / 4 then, else 0),
// the rest element by element; a grid-stride loop over a grid sized to the chip, no LDS in the data path.  `a` and `out` may be one
// buffer (every element is read and written by the same thread), so neither carries __restrict__.
// The ReLU is `r > 0 ? r : 0`: what bn.hip's fmaxf(v, 0.f), which this pass replaces, gives -- a NaN sum becomes 0 (torch.relu keeps it)
// and -0.0 becomes +0.0.  Deliberate: the frozen route answers as the eval route does.  Without RELU the sum is stored as it is.
template <bool RELU>
__global__ __launch_bounds__(TPB) void add_relu_kernel(const float* a, const float* __restrict__ b, float* out, long n4, long n,
                                                       unsigned* __restrict__ amax) {
    const long tid = (long)blockIdx.x * TPB + threadIdx.x, nth = (long)gridDim.x * TPB;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    float4* o4 = reinterpret_cast<float4*>(out);
    float mx = 0.f;                      // largest |out| this thread wrote (-> amax_out: the operand scale of the convolution that reads it)
    for (long i = tid; i < n4; i += nth) {
        const float4 x = a4[i], y = b4[i];
        float4 r = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
        if (RELU) { r.x = r.x > 0.f ? r.x : 0.f; r.y = r.y > 0.f ? r.y : 0.f; r.z = r.z > 0.f ? r.z : 0.f; r.w = r.w > 0.f ? r.w : 0.f; }
        o4[i] = r;
        mx = fmaxf(fmaxf(mx, fmaxf(jp_fmag(r.x), jp_fmag(r.y))), fmaxf(jp_fmag(r.z), jp_fmag(r.w)));
    }
    for (long i = (n4 << 2) + tid; i < n; i += nth) {
        float r = a[i] + b[i];
        if (RELU) r = r > 0.f ? r : 0.f;
        out[i] = r;
        mx = fmaxf(mx, jp_fmag(r));
    }
    jp_block_amax_commit(mx, amax);      // wave shuffles, one word per wave, ONE atomicMax per workgroup into its way of the slot (as scale.hip)
}
}  // namespace

// ---- C ABI (include/jperceiver_hip.h)
extern "C" int jp_bn_fold_conv(const float* w, const float* conv_bias, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, float eps, float* w_out, float* bias_out, int Cout, int K, void* stream) {
    JP_CHECK_ARG(w && gamma && beta && running_mean && running_var && w_out && bias_out, "bn_fold_conv: null pointer");
    JP_CHECK_ARG(Cout > 0 && K > 0, "bn_fold_conv: Cout and K must be positive");
    JP_CHECK_ARG(eps >= 0.f, "bn_fold_conv: eps must not be negative");
    hipLaunchKernelGGL(bn_fold_conv_kernel, dim3(Cout), dim3(TPB), 0, static_cast<hipStream_t>(stream), w, conv_bias, gamma, beta,
                       running_mean, running_var, eps, w_out, bias_out, K);
    JP_LAUNCH_CHECK();
}

// amax_out: optional magnitude slot (see the header) that receives max |out|
extern "C" int jp_add_relu(const float* a, const float* b, float* out, long n, int relu, float* amax_out, void* stream) {
    JP_CHECK_ARG(a && b && out, "add_relu: null pointer");
    JP_CHECK_ARG(n > 0, "add_relu: n must be positive");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool al = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long n4 = al ? n >> 2 : 0;
    // 256 CUs x 8 workgroups of 4 waves: every SIMD is full, the rest of the tensor is walked by the grid-stride loop
    const int blocks = (int)std::min<long>(((al ? n4 + (n & 3) : n) + TPB - 1) / TPB, 2048);
    unsigned* am = reinterpret_cast<unsigned*>(amax_out);
    jp_prof_before("jp_add_relu", 0.0, st);          // (a no-op unless a profile is open; 0 FLOPs: no GEMM, the record carries the time)
    if (relu)
        hipLaunchKernelGGL(add_relu_kernel<true>, dim3(blocks), dim3(TPB), 0, st, a, b, out, n4, n, am);
    else
        hipLaunchKernelGGL(add_relu_kernel<false>, dim3(blocks), dim3(TPB), 0, st, a, b, out, n4, n, am);
    jp_prof_after(st);
    JP_LAUNCH_CHECK();
}
