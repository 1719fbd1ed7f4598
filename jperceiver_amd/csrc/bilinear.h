// The half-pixel bilinear sampling of jp_bilinear_fwd (F.interpolate(mode='bilinear', align_corners=False)), shared by every kernel
// whose result must carry the same bits: pointwise.hip's bilinear_fwd_kernel and stream.hip's pose-pair kernel.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void bil_src(int o, float scale, int in, int& i0, int& i1, float& w1) {
    float src = ((float)o + 0.5f) * scale - 0.5f;   // PyTorch area_pixel_compute_source_index
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    w1 = src - (float)i0;
}

// output pixel (oy, ox) of one H x W plane `xp`; sy = (float)H / OH, sx = (float)W / OW as the entry points form them
__device__ __forceinline__ float bil_sample(const float* __restrict__ xp, int oy, int ox, int H, int W, float sy, float sx) {
    int y0, y1, x0, x1;
    float wy, wx;
    bil_src(oy, sy, H, y0, y1, wy);
    bil_src(ox, sx, W, x0, x1, wx);
    const float a = xp[y0 * W + x0], b = xp[y0 * W + x1], c = xp[y1 * W + x0], d = xp[y1 * W + x1];
    return (1.f - wy) * ((1.f - wx) * a + wx * b) + wy * ((1.f - wx) * c + wx * d);
}
