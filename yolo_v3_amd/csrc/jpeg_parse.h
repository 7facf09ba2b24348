// Host side of the JPEG decoder (plain C++, no HIP): yv3_jpeg_parse and yv3_jpeg_workspace_bytes are declared in yv3.h;
// this header adds what jpeg.hip shares with them.
#pragma once
#include "jpeg_entropy.h"

// The workspace of a batch: B of these records first (256-aligned as a whole), then each image's share in batch order.
struct yv3_jpeg_slot {
    long long coef_off, plane_off, unit_off;     // byte offsets into the workspace
    int status;
    int prog;                                    // 1: a progressive image (yv3_jpeg_decode_batch_prog), entropy_prog_kernel's
};

// Workspace bytes of a batch from its host records; with `strict`, a record yv3_jpeg_geometry refuses makes the result 0.
size_t yv3_jpeg_batch_workspace(const yv3_jpeg_info* infos, int B, bool strict);

// The workspace of yv3_jpeg_decode_batch_prog with P > 0: the B slot records, a copy of the B info records in which every
// progressive image's is a frame record (yv3_jpegp_as_frame; both 256-aligned as a whole), then each image's share.
// 0 for a record or an index that is refused.
size_t yv3_jpeg_batch_workspace_prog(const yv3_jpeg_info* infos, const int* prog_of, const yv3_jpeg_prog* progs, int P, int B,
                                     long long* max_blocks, long long* max_groups);
