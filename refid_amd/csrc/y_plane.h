// The BT.601 Y plane of the reference's to_y_channel (basicsr/metrics/metric_util.py) after astype(float32), shared by
// niqe.hip and score.hip so that NIQE and the Y-channel PSNR / SSIM see the same bits:
//   v_c = fl32(u8 / 255);  y64 = ((b*24.966 + g*128.553) + r*65.481) + 16.0 in float64;  Y = fl32(fl32(y64 / 255.0) * 255)
// Every step is one correctly rounded operation: contraction is off inside the body whatever the including file sets.
// tests/niqe_ref.py::y_plane restates it.
#pragma once
#include <hip/hip_runtime.h>

// r, g, b: the channels' uint8 values as floats (exact)
__device__ __forceinline__ float refid_y601_u8(float r_u8, float g_u8, float b_u8) {
#pragma clang fp contract(off)
    const double r = __fdiv_rn(r_u8, 255.f), g = __fdiv_rn(g_u8, 255.f), b = __fdiv_rn(b_u8, 255.f);
    const double y64 = ((b * 24.966 + g * 128.553) + r * 65.481) + 16.0;
    return (float)(y64 / 255.0) * 255.f;
}
