// color_convert.hpp -- the integer colour arithmetic of the colour-frame decode (colorframes.hip), in one
// place: the kernels, mqr_color_constants (which hands the constants to mqr/colorframes.py's host path) and
// nothing else use it.
//
// PROVENANCE: the three pieces below restate OpenCV 4.x (imgproc: color_yuv.simd.hpp, color_rgb.simd.hpp,
// deriv.cpp) AS RECALLED.  OpenCV was not available when this was written, so their parity with OpenCV is
// UNPINNED: a fixture recorded from a real OpenCV (cv2.cvtColor COLOR_YUV2BGR_I420 / COLOR_BGR2GRAY,
// cv2.Laplacian ksize = 1) pins or corrects them here, and only here.
//
//   I420 -> BGR (ITU-R BT.601, 20-bit fixed point, one (U,V) pair per 2x2 block, no chroma interpolation)
//       y = max(0, Y - 16) * CY,  u = U - 128,  v = V - 128,  rnd = 1 << 19
//       r = sat8((y + CVR*v + rnd) >> 20)
//       g = sat8((y + CVG*v + CUG*u + rnd) >> 20)
//       b = sat8((y + CUB*u + rnd) >> 20)
//   BGR -> grey (15-bit fixed point)
//       grey = (3735*B + 19235*G + 9798*R + (1 << 14)) >> 15
//   Laplacian, ksize = 1: [[0,1,0],[1,-4,1],[0,1,0]] on the integer grey values, border reflect-101
//       (index -1 -> 1, n -> n - 2); each value lies in [-1020, 1020].
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mqr {
namespace cc {

constexpr int kCY = 1220542, kCUB = 2116026, kCUG = -409993, kCVG = -852492, kCVR = 1673527;
constexpr int kYuvShift = 20;
constexpr int kGreyB = 3735, kGreyG = 19235, kGreyR = 9798, kGreyShift = 15;
constexpr int kLapMax = 1020;  // |Laplacian| <= 4 * 255

__host__ __device__ inline int sat8(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }

// The chroma terms of one (U,V) pair, rounding term included; shared by the pair's four pixels.
struct Chroma {
    int r, g, b;
};
__host__ __device__ inline Chroma chroma_terms(int U, int V) {
    const int u = U - 128, v = V - 128, rnd = 1 << (kYuvShift - 1);
    return {rnd + kCVR * v, rnd + kCVG * v + kCUG * u, rnd + kCUB * u};
}
// One pixel -> r | g << 8 | b << 16.  (>> of a negative int is arithmetic here, as in OpenCV's build.)
__host__ __device__ inline uint32_t yuv_to_rgb(int Y, const Chroma& c) {
    const int y = (Y > 16 ? Y - 16 : 0) * kCY;
    return (uint32_t)sat8((y + c.r) >> kYuvShift) | (uint32_t)sat8((y + c.g) >> kYuvShift) << 8 |
           (uint32_t)sat8((y + c.b) >> kYuvShift) << 16;
}
__host__ __device__ inline int grey_of(int r, int g, int b) {
    return (kGreyB * b + kGreyG * g + kGreyR * r + (1 << (kGreyShift - 1))) >> kGreyShift;
}
// border reflect-101 of index i into [0, n), for -1 <= i <= n and n >= 2
__host__ __device__ inline int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

}  // namespace cc
}  // namespace mqr
