/*
 * ovn_hip_deskew.h -- the extension of the C ABI of libovn_hip.so (include/ovn_hip.h) that undoes the sensor's motion within a sweep.
 *
 * The entry points of this header are ADDITIONS to the library: the tables that pin the functions of ovn_hip.h (tests/test_abi.py,
 * tests/test_engine_calls_host.py) could not be edited by the change that added them, so they are declared here, bound from
 * `_lib.EXT_SIGNATURES` and guarded by tests/test_deskew_host.py.  OVN_ABI_VERSION does not change: nothing that existed changed.
 *
 * The conventions are those of ovn_hip.h: "dev" pointers are device memory owned by the caller; `stream` is a hipStream_t passed as
 * void* (NULL = the legacy default stream) and a call only ENQUEUES work on it; the context's device is selected for the call's
 * duration and the caller's current device restored; 0 = success, else an error whose message ovn_last_error() returns.  `stream` is
 * the SECOND parameter, as in ovn_tsdf_raycast; tests/test_gpu_deskew_stream.py runs the call on a non-default stream.
 */
#ifndef OVN_HIP_DESKEW_H
#define OVN_HIP_DESKEW_H

#include "ovn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ovn_deskew: every point of a raw sweep moved into the sensor frame of ONE instant of that sweep (csrc/deskew.hip; DESIGN.md
 * section 37).  A spinning sensor measures the points of a sweep one after the other while it moves; with the sensor's motion over the
 * sweep given as a constant body-frame twist, this call re-expresses each point in the frame the sensor had at time fraction t_ref.
 *   points_dev   (total,4) f32: x, y, z, intensity of the concatenated scans, 16-byte aligned
 *   offsets_dev  (n_scans+1) int64, ascending: scan s is rows offsets[s] .. offsets[s+1] - 1 of points_dev (absolute row numbers, as for
 *                ovn_project: a slice of a longer offsets array handles that range of scans).  Rows outside offsets[0] .. offsets[n_scans]
 *                are neither read nor written
 *   times_dev    NULL, or (total) f32, indexed like the rows of points_dev: the time fraction s of each point within its sweep, 0 the
 *                sweep's first point and 1 its last.  Values outside 0 .. 1 extrapolate (packet jitter is real)
 *   start_azimuth_deg, clockwise: the time source when times_dev is NULL (ignored, but still checked, when it is given).  With
 *                yaw = -atan2f(y, x) (the projection's yaw), q = yaw / (float)pi, c = 0.5f * (q + 1.0f), and c0 = (float)(0.5 *
 *                (start_azimuth_deg / 180 + 1)) formed in fp64: d = c - c0 for clockwise = 1 (yaw grows with time: the sensor turns
 *                clockwise seen from above), d = c0 - c for clockwise = 0, and s = d - floorf(d).  atan2f is the device library's own:
 *                this route is NOT the NumPy-exact arctangent of ovn_project and makes no bit-exactness claim against NumPy.  A point
 *                at the seam (yaw = start azimuth) belongs to either end of the sweep by nature; nothing is done about it
 *   twists_dev   (n_scans,6) f64: row s is the sensor's body-frame twist xi = (v, omega) over ONE WHOLE sweep of scan s, in the
 *                library's twist order (translation first).  The sensor pose at fraction s is T(t_ref) Exp((s - t_ref) xi)
 *   t_ref        the fraction whose sensor frame the output is expressed in, rounded to f32 (that f32 value IS the t_ref of the model)
 *   out_points_dev (total,4) f32, 16-byte aligned, rows as in points_dev.  out_points_dev == points_dev (in place) is allowed; any other
 *                overlap of the two row ranges is the caller's promise not to make (the library does not know `total`)
 * Model: a point p measured at fraction s, with tau = s - t_ref, a = tau |omega|, k = omega / |omega| and K = [k]x, becomes
 *   p' = R p + t,   R = I + sin a K + (1 - cos a) K^2,   t = tau (I + ((1 - cos a) / a) K + ((a - sin a) / a) K^2) v
 * Per scan, in fp64, each result rounded to f32 once: th = sqrt((w0 w0 + w1 w1) + w2 w2), k = omega / th (0 when th == 0), v,
 * kv = k x v, kkv = k x kv (the cross products from the fp64 k).  Per point, every operation ONE f32 operation rounded on its own
 * (no FMA contraction), cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
 *   1  tau = s - t_ref;  a = tau * th
 *   2  sa = sinf(a);  sh = sinf(0.5f * a);  c1 = (2.0f * sh) * sh                       [sin a and 1 - cos a, the latter without cancellation]
 *   3  |a| <  2^-6:  aa = a * a;  B = a * (0.5f - aa / 24.0f);  C = aa * ((1.0f / 6.0f) - aa / 120.0f)   [the series; next terms < 2^-39]
 *      |a| >= 2^-6:  B = c1 / a;  C = (a - sa) / a
 *   4  kp = cross(k, p);  kkp = cross(k, kp);  r = (p + sa * kp) + c1 * kkp
 *   5  u = (v + B * kv) + C * kkv;  t = tau * u;  p' = r + t;  the intensity is copied
 * sinf is the device library's; the NumPy restatement (tests/_deskew_ref.py) follows the sequence with its own sine and serves for
 * error bounds, not for bits.
 * Special cases: a scan whose twist is six zeros (of either sign) is copied bit for bit -- a branch per scan, so -0.0 and NaN payloads
 * stay; a scan whose twist has a non-finite entry is copied bit for bit as well (no motion estimate is better than a wrong one); a point
 * whose time is not finite (given, or from a non-finite x or y) is written as (0, 0, 0, intensity), which every projection drops.
 * One thread per point in a grid-stride loop over rows offsets[0] .. offsets[n_scans] - 1, the scan of a row found by bisection of
 * offsets_dev, one 16-byte load and one 16-byte store per point, all index arithmetic in 64 bits, no atomics, no scratch of the
 * context.  A point's result depends on its row's values and its scan's twist alone: a scan has the same bits alone and at any position
 * of any batch, and the same arguments give the same bits.
 * OVN_ERR_ARG, before any launch (the output is untouched): a NULL ctx; n_scans < 0; a t_ref that is not finite (before or after
 * rounding to f32) or a non-finite start_azimuth_deg; clockwise outside {0, 1}; and for n_scans > 0 a NULL points_dev, offsets_dev,
 * twists_dev or out_points_dev, or a points_dev or out_points_dev that is not 16-byte aligned.  n_scans == 0 is a no-op. */
int ovn_deskew(ovn_ctx* ctx, void* stream, const float* points_dev, const int64_t* offsets_dev, int n_scans, const float* times_dev,
               double start_azimuth_deg, int clockwise, const double* twists_dev, double t_ref, float* out_points_dev);

#ifdef __cplusplus
}
#endif

#endif /* OVN_HIP_DESKEW_H */
