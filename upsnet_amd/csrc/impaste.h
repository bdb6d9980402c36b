// impaste.h -- the im_post paste rule (upsnet/upsnet_end2end_test.py:95-152) for device code, shared by postprocess.hip
// (im_post_rle_kernel: RLE of each pasted mask) and det_eval.hip (bit planes of the pasted masks for mask AP).
// A detection's MxM mask probability of its class is zero-padded to (M+2)x(M+2), resized (cv2 INTER_LINEAR) to the box expanded by
// (M+2)/M and truncated to integers, thresholded at 0.5 and pasted into the image: pixel (x, y) is set iff x_0 <= x < x_1,
// y_0 <= y < y_1 and pan_resize_at(s_pad, M + 2, w, h, x - bx0, y - by0) > 0.5f.
#pragma once
#include "resize.h"

#define IMP_MAXMS 34   // padded mask side (28 + 2 in every config)

struct ImpBox { int bx0, by0, w, h, x_0, x_1, y_0, y_1; };

// zero-padded mask of detection d (channel cls_inds[d] when num_ch > 1) into s_pad[(ms+2)^2]; threads tid, tid + nt, ...
__device__ static inline void imp_load_pad(float *__restrict__ s_pad, const float *__restrict__ mask_prob, const int64_t *__restrict__ cls_inds,
                                           const int d, const int num_ch, const int ms, const int tid, const int nt)
{
    const int ps = ms + 2;
    const int ch = num_ch > 1 ? (int)cls_inds[d] : 0;
    const float *src = mask_prob + ((long)d * num_ch + ch) * ms * ms;
    for (int i = tid; i < ps * ps; i += nt) {
        const int py = i / ps, px = i - py * ps;
        s_pad[i] = (py >= 1 && py <= ms && px >= 1 && px <= ms) ? src[(py - 1) * ms + (px - 1)] : 0.f;
    }
}

// expand_boxes (bbox_transform.py:365-381) in float32, then astype(int32) (truncation); box = (x1, y1, x2, y2) float32
__device__ static inline ImpBox imp_box(const float *__restrict__ box, const int ms, const int H, const int W)
{
    const float scale = (float)(((double)ms + 2.0) / (double)ms);
    const float bx1 = box[0], by1 = box[1], bx2 = box[2], by2 = box[3];
    float w_half = (bx2 - bx1) * .5f, h_half = (by2 - by1) * .5f;
    const float x_c = (bx2 + bx1) * .5f, y_c = (by2 + by1) * .5f;
    w_half = w_half * scale; h_half = h_half * scale;
    const int rx1 = (int)(x_c - w_half), rx2 = (int)(x_c + w_half), ry1 = (int)(y_c - h_half), ry2 = (int)(y_c + h_half);
    ImpBox b;
    b.w = max(rx2 - rx1 + 1, 1); b.h = max(ry2 - ry1 + 1, 1);
    b.bx0 = rx1; b.by0 = ry1;
    b.x_0 = max(rx1, 0); b.x_1 = min(rx2 + 1, W);
    b.y_0 = max(ry1, 0); b.y_1 = min(ry2 + 1, H);
    return b;
}
