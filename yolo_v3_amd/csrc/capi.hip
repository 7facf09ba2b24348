// C-ABI glue: version / error strings and the dtype dispatch of the convolution entry points.
#include "yv3_common.h"

extern "C" int yv3_version(void) { return YV3_VERSION; }

extern "C" const char* yv3_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case YV3_EINVAL: return "invalid argument (null pointer or non-positive size)";
        case YV3_ESHAPE: return "shape not supported by this kernel family";
        case YV3_EWORKSPACE: return "workspace too small";
        case YV3_EDTYPE: return "unknown dtype";
        case YV3_ERCCL: return "RCCL: librccl.so not found or ncclAllGather failed";
        case YV3_ELIMIT: return "input beyond a documented kernel limit";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown yv3 error";
    }
}

static int check_desc(const yv3_conv_desc* d, bool need_output = true) {
    if (!d || !d->x || !d->w || !d->beta || (need_output && !d->y && !d->dec_out)) return YV3_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->cin <= 0 || d->cout <= 0) return YV3_EINVAL;
    if (d->k != 1 && d->k != 3) return YV3_ESHAPE;
    if (d->stride != 1 && d->stride != 2) return YV3_ESHAPE;
    if (d->k == 1 && d->stride != 1) return YV3_ESHAPE;
    if (d->cin % 32 != 0 || d->cout_pad % 32 != 0 || d->cout_pad < d->cout) return YV3_ESHAPE;
    if (d->cin_up) {
        if (d->k != 1 || !d->x2 || d->cin_up % 32 != 0 || d->cin_up >= d->cin) return YV3_ESHAPE;
        if ((d->H & 1) || (d->W & 1)) return YV3_ESHAPE;
    }
    return 0;
}

static int plane_count(int dtype) {
    return dtype == YV3_BF16 || dtype == YV3_F16 || dtype == YV3_I8 ? 1 : dtype == YV3_F32_F16X2 ? 2 : dtype == YV3_F32_BF16X3 ? 3 : 0;
}

// The dtype / output-format errors of yv3_conv2d: ONE function, called by the launch and by the form query, so that
// yv3_conv2d_form returns "the YV3_E* code yv3_conv2d would return" (include/yv3.h).
static int check_dtype(const yv3_conv_desc* d) {
    if (d->dtype == YV3_F32) {
        if (d->out_dtype != YV3_F32) return YV3_EDTYPE;
        if (d->dec_out) return YV3_EDTYPE;                     // the fused decode lives in the plane kernels' epilogue
        return 0;
    }
    if (d->dtype == YV3_I8) return (d->out_dtype == YV3_I8 || d->out_dtype == YV3_BF16) && !d->dec_out ? 0 : YV3_EDTYPE;   // (the quantised integers as int8, or as one bf16 plane)
    if (plane_count(d->dtype)) return d->out_dtype != YV3_F32 && d->out_dtype != d->dtype ? YV3_EDTYPE : 0;
    return YV3_EDTYPE;
}

// yv3_conv2d and its three queries: the argument checks, ONE CU-count query, ONE call of the selector (conv_select.cpp), which is the CU
// count's only reader -- then launch its choice or report its form / its number of launches / its description (or the YV3_E* code the
// launch would return)
enum { CONV_LAUNCH, CONV_FORM, CONV_LAUNCHES, CONV_KERNEL };
static int conv2d(const yv3_conv_desc* d, int what, hipStream_t s, char* buf = nullptr, size_t buf_bytes = 0) {
    int rc = check_desc(d, what == CONV_LAUNCH);    // (the queries: a fused-decode head may not have its output bound yet)
    if (!rc) rc = check_dtype(d);
    if (rc) return rc;
    const int ncu = yv3_num_cu(), np = plane_count(d->dtype);
    if (d->dtype == YV3_F32) {
        const yv3_f32_choice c = yv3_select_f32(d, ncu);
        return c.rc ? c.rc : what == CONV_FORM ? c.form : what == CONV_LAUNCHES ? c.launches : what == CONV_KERNEL ? yv3_describe_f32(c, buf, buf_bytes) : yv3_conv2d_f32(d, c, s);
    }
    const yv3_planes_choice c = d->dtype == YV3_I8 ? yv3_select_planes_i8(d, ncu) : yv3_select_planes(d, np, ncu);
    return c.rc ? c.rc : what == CONV_FORM ? c.form : what == CONV_LAUNCHES ? c.launches : what == CONV_KERNEL ? yv3_describe_planes(c, buf, buf_bytes) :
           d->dtype == YV3_F16 ? yv3_conv2d_planes_f16(d, c, s) : d->dtype == YV3_I8 ? yv3_conv2d_planes_i8(d, c, s) :
           yv3_conv2d_planes(d, np, c, s);      // (one plane either way: the element type picks the launcher)
}
extern "C" int yv3_conv2d(const yv3_conv_desc* d, void* stream) { return conv2d(d, CONV_LAUNCH, (hipStream_t)stream); }
extern "C" int yv3_conv2d_form(const yv3_conv_desc* d) { return conv2d(d, CONV_FORM, nullptr); }
extern "C" int yv3_conv2d_launches(const yv3_conv_desc* d) { return conv2d(d, CONV_LAUNCHES, nullptr); }
extern "C" int yv3_conv2d_kernel(const yv3_conv_desc* d, char* buf, size_t buf_bytes) { return conv2d(d, CONV_KERNEL, nullptr, buf, buf_bytes); }

extern "C" int yv3_conv2d_sequence(const yv3_conv_desc* descs, int n, void* stream) {
    if (!descs || n < 0) return YV3_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int rc = yv3_conv2d(&descs[i], stream);
        if (rc) return rc;
    }
    return 0;
}
