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

// Workspace bytes of a batch from its host records: the B slot records, with P > 0 a copy of the B info records in which every
// progressive image's is a frame record (yv3_jpegp_as_frame; both 256-aligned as a whole), then each image's share.  P == 0:
// every image is a baseline one, prog_of and progs are not looked at, and a record yv3_jpeg_geometry refuses is skipped, or with
// `strict` makes the result 0.  P > 0: always strict, and 0 too for a prog_of entry outside [-1, P).  max_blocks / max_groups
// (or null): raised to the largest image's blocks and groups of four pixels, which size the grids of idct_kernel and colour_kernel.
size_t yv3_jpeg_batch_workspace(const yv3_jpeg_info* infos, int B, const int* prog_of, const yv3_jpeg_prog* progs, int P, bool strict,
                                long long* max_blocks, long long* max_groups);
