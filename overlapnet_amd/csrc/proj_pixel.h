// The spherical projection of ONE point (utils.py:75-104): shared by projection.hip (points of a scan) and tsdf.hip (samples of a
// volume seen from a sensor), so that both put a point into the same pixel from the same float32 operations.  Include only from files
// compiled with -ffp-contract=off: every operation below rounds on its own, as NumPy's float32 code does.
#pragma once

#include "svml_f32.h"

#include <cmath>

struct ProjGeom {
  int H, W;
  float fov_down_abs;  // float32(|fov_down| in radians)
  float fov;           // float32(|fov_down| + |fov_up|)
  float max_range;
  int trig;            // 0: NumPy's float32 arctan2 / arcsin on AVX512_SKX x86-64 (SVML, svml_f32.h); 1: the correctly rounded float32
                       // results (float64 function rounded once) -- what a host whose NumPy calls a correctly rounded libm produces
};

__device__ __forceinline__ float point_depth(float x, float y, float z) {
  return sqrtf((x * x + y * y) + z * z);                       // utils.py:75
}

// utils.py:86-95 for a point of depth > 0: both angles and the pixel coordinates before floor and clamp
__device__ __forceinline__ void point_to_subpixel(float x, float y, float z, float depth, const ProjGeom& gm, float& yaw, float& pitch,
                                                  float& px, float& py) {
  if (gm.trig == 0) {
    yaw = -ovn_svml::atan2f_np(y, x);                          // utils.py:86  (np.arctan2 on float32: svml_f32.h)
    pitch = ovn_svml::asinf_np(z / depth);                     // utils.py:87  (np.arcsin on float32)
  } else {                                                     // ovn_set_projection_trig(ctx, 1)
    yaw = -(float)atan2((double)y, (double)x);
    pitch = (float)asin((double)(z / depth));
  }
  px = 0.5f * (yaw / 3.14159274101257324f + 1.0f);             // utils.py:90
  py = 1.0f - (pitch + gm.fov_down_abs) / gm.fov;              // utils.py:91
  px = px * (float)gm.W;                                       // utils.py:94
  py = py * (float)gm.H;                                       // utils.py:95
}

// the column of an unfloored px: utils.py:98-100
__device__ __forceinline__ float clamp_column(float px, const ProjGeom& gm) {
  return fmaxf(0.0f, fminf((float)(gm.W - 1), floorf(px)));
}

// utils.py:75-104 for one point: depth, the range filter, both angles and the pixel.  false = dropped by the filter.
__device__ __forceinline__ bool point_to_pixel(float x, float y, float z, const ProjGeom& gm, float& depth, float& yaw, float& pitch,
                                               int& pix) {
  depth = point_depth(x, y, z);
  yaw = pitch = 0.f;
  pix = 0;
  if (!((depth > 0.0f) && (depth < gm.max_range))) return false;   // utils.py:76-77
  float px, py;
  point_to_subpixel(x, y, z, depth, gm, yaw, pitch, px, py);
  px = clamp_column(px, gm);                                   // utils.py:98-100
  py = fmaxf(0.0f, fminf((float)(gm.H - 1), floorf(py)));      // utils.py:102-104
  pix = (int)py * gm.W + (int)px;
  return true;
}

// same double arithmetic as utils.py:70-72, then the float32 casts NumPy applies to the scalars
static inline ProjGeom make_geom(int H, int W, double fov_up_deg, double fov_down_deg, double max_range, int trig) {
  const double up = fov_up_deg / 180.0 * 3.14159265358979323846;
  const double down = fov_down_deg / 180.0 * 3.14159265358979323846;
  ProjGeom gm;
  gm.H = H;
  gm.W = W;
  gm.fov_down_abs = (float)fabs(down);
  gm.fov = (float)(fabs(down) + fabs(up));
  gm.max_range = (float)max_range;
  gm.trig = trig;
  return gm;
}
