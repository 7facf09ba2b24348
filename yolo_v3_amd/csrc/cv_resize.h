// OpenCV's fixed-point resize arithmetic, shared by prepost.hip (letterbox / resize kernels) and augment.hip (training
// augmentation).  Include inside an anonymous namespace; the including translation unit must be compiled with -ffp-contract=off.
#pragma once

// cv2.resize for CV_8U, fixed-point path (OpenCV modules/imgproc/src/resize.cpp; cv2 itself is absent from this
// environment, so parity with it is UNPINNED -- the CPU oracle restates exactly this integer algorithm and the
// kernels match it bit for bit):
//   coordinates   fx = (float)((dx + 0.5) * scale - 0.5), scale = 1 / ((double)dst / src); sx = floor(fx); fx -= sx
//   INTER_CUBIC   interpolateCubic (A = -0.75, float32, source operation order) -> saturate_cast<short>(c * 2048);
//                 HResizeCubic: int32 sum of 4 taps (replicated border); VResizeCubic + FixedPtCast<int,uchar,22>:
//                 saturate_cast<uchar>((sum + (1 << 21)) >> 22)
//   INTER_LINEAR  (1 - fx, fx) * 2048 as shorts, edge clamps; VResizeLinear<uchar,int,short>:
//                 uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2); exact 2x2 down-scale ->
//                 INTER_AREA (a + b + c + d + 2) >> 2
// (the float32 coefficient arithmetic must not fuse: the including translation unit is compiled with -ffp-contract=off)
__device__ inline void cv_coord(int d, double scale, int& s, float& f) {
    const float fx = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(fx);
    f = fx - (float)s;
}
__device__ inline int cv_short(float c) {                      // saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE)
    return min(max((int)rintf(c * 2048.f), -32768), 32767);
}
__device__ inline void cv_cubic_coeffs(float x, int c[4]) {
    const float A = -0.75f;
    float w[4];
    w[0] = ((A * (x + 1.f) - 5.f * A) * (x + 1.f) + 8.f * A) * (x + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    w[2] = ((A + 2.f) * (1.f - x) - (A + 3.f)) * (1.f - x) * (1.f - x) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = cv_short(w[k]);
}
