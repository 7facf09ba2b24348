// Box outlines and label tags on a batch of uint8 RGB images, in place (yv3_draw_boxes of include/yv3.h).
// One thread per pixel: it walks its image's boxes in detection order and keeps the colour of the last box whose outline or tag
// covers it, so overlapping boxes come out as if painted one after the other, without atomics.  The kernel knows no font: tags are
// 1-bit masks the caller rasterised.
#include "yv3_common.h"

namespace {

__global__ void __launch_bounds__(256) draw_boxes_kernel(const yv3_draw_image* __restrict__ images, const yv3_draw_box* __restrict__ boxes,
                                                         int num_boxes_total, const yv3_draw_tag* __restrict__ tags, int num_tags,
                                                         const unsigned char* __restrict__ atlas, long long atlas_bytes, int t) {
    const yv3_draw_image im = images[blockIdx.y];
    if (im.num_boxes <= 0 || im.width <= 0 || im.height <= 0 || !im.pixels || im.pitch < (long long)im.width * 3) return;
    if (im.first_box < 0 || (long long)im.first_box + im.num_boxes > num_boxes_total) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)im.width * im.height) return;
    const int x = (int)(i % im.width), y = (int)(i / im.width), W = im.width, H = im.height;
    bool painted = false;
    unsigned char r = 0, g = 0, b = 0;
    for (int j = 0; j < im.num_boxes; ++j) {
        const yv3_draw_box box = boxes[im.first_box + j];
        if (x >= box.x1 && x <= box.x2 && y >= box.y1 && y <= box.y2 &&
            ((long long)x - box.x1 < t || (long long)box.x2 - x < t || (long long)y - box.y1 < t || (long long)box.y2 - y < t)) {
            painted = true;
            r = box.rgb[0], g = box.rgb[1], b = box.rgb[2];
        }
        if (box.tag < 0 || box.tag >= num_tags) continue;
        const yv3_draw_tag tag = tags[box.tag];
        if (tag.width <= 0 || tag.height <= 0) continue;
        const long long left = max(min(max((long long)box.x1, 0LL), (long long)W - tag.width), 0LL);
        const long long bottom = min(max((long long)box.y1, (long long)tag.height), (long long)H), top = bottom - tag.height;
        if (x < left || x >= left + tag.width || y < top || y >= bottom) continue;
        const long long row_bytes = (tag.width + 7) / 8, at = tag.offset + (y - top) * row_bytes + (x - left) / 8;
        if (tag.offset < 0 || at >= atlas_bytes) continue;
        const bool ink = (atlas[at] >> (7 - (int)((x - left) & 7))) & 1;
        painted = true;
        r = ink ? 0 : box.rgb[0], g = ink ? 0 : box.rgb[1], b = ink ? 0 : box.rgb[2];
    }
    if (painted) {
        unsigned char* p = im.pixels + (long long)y * im.pitch + (long long)x * 3;
        p[0] = r, p[1] = g, p[2] = b;
    }
}

}  // namespace

extern "C" int yv3_draw_boxes(const yv3_draw_image* images, int B, const yv3_draw_box* boxes, int num_boxes_total, const yv3_draw_tag* tags,
                              int num_tags, const unsigned char* atlas, long long atlas_bytes, int thickness, int max_width, int max_height,
                              void* stream) {
    if (!images || B < 1 || B > 65535 || num_boxes_total < 0 || num_tags < 0 || atlas_bytes < 0 || thickness < 1 || max_width < 1 || max_height < 1)
        return YV3_EINVAL;
    if ((num_boxes_total && !boxes) || (num_tags && (!tags || !atlas))) return YV3_EINVAL;
    if (num_boxes_total == 0) return 0;
    const long long pixels = (long long)max_width * max_height;
    if ((pixels + 255) / 256 > 0x7fffffffLL) return YV3_ELIMIT;
    hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)((pixels + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, images, boxes,
                       num_boxes_total, tags, num_tags, atlas, atlas_bytes, thickness);
    YV3_CHECK_LAUNCH();
    return 0;
}
