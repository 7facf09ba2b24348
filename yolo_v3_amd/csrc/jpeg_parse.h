// Host side of the JPEG decoder (plain C++, no HIP): yv3_jpeg_parse and yv3_jpeg_workspace_bytes are declared in yv3.h;
// this header adds what jpeg.hip shares with them.
#pragma once
#include "jpeg_entropy.h"

// The workspace of a batch: B of these records first (256-aligned as a whole), then each image's share in batch order.
struct yv3_jpeg_slot {
    long long coef_off, plane_off, unit_off;     // byte offsets into the workspace
    int status, pad;
};

// Workspace bytes of a batch from its host records; with `strict`, a record yv3_jpeg_geometry refuses makes the result 0.
size_t yv3_jpeg_batch_workspace(const yv3_jpeg_info* infos, int B, bool strict);
