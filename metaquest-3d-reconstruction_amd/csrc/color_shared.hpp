// color_shared.hpp -- what the colour assignment (color.hip) and the colour-map optimiser (colormap.hip)
// share: the keyframe camera record, the depth-boundary masks and the step from per-vertex float64
// averages to the output colours (seen vertices, k-nearest-neighbour fill of the rest).  The kernels live
// in color.hip; these host functions enqueue them, so both entry points run the same code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mqr {

struct ColorCam {
    double E[12];  // world -> camera, rows 0..2 of T_wc
    double fx, fy, cx, cy;
};

inline void fill_color_cams(const double* K, const double* T_wc, int N, ColorCam* cams) {
    for (int c = 0; c < N; ++c) {
        for (int k = 0; k < 12; ++k) cams[c].E[k] = T_wc[16 * c + k];
        cams[c].fx = K[9 * c + 0];
        cams[c].fy = K[9 * c + 4];
        cams[c].cx = K[9 * c + 2];
        cams[c].cy = K[9 * c + 5];
    }
}

// The depth-boundary masks of N keyframes (k_cm_filter_h, k_cm_filter_v, k_cm_dilate) on stream s: t_hit
// [N][H][W] -> mask (255 = near a depth discontinuity).  hx, hy (float) and m0 (uint8) are NHW-element
// scratch planes.  Nothing is enqueued when NHW == 0.
void cm_enqueue_masks(hipStream_t s, const float* t_hit, int64_t NHW, int H, int W, float depth_trunc,
                      double disc_threshold, int half_dilation, float* hx, float* hy, uint8_t* m0, uint8_t* mask);

// From the float64 averages `avg` [nv][3] and sample counts `cnt` [nv] (device) to the colours `out`
// [nv][3] (device): a sampled vertex takes its average, every other vertex the float64 mean of its knn
// nearest sampled vertices' averages (0 when knn == 0 or nothing is sampled).  Synchronises s.  Returns 0,
// or 1 with the error set (prefixed by `who`).
int cm_finish_colors(int device, hipStream_t s, const float* V, int64_t nv, const double* avg, const int32_t* cnt,
                     int knn, float* out, const char* who);

}  // namespace mqr
