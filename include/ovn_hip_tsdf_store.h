/*
 * ovn_hip_tsdf_store.h -- the extension of the C ABI of libovn_hip.so (include/ovn_hip.h) that moves whole 8 x 8 x 8 bricks between the
 * rolling TSDF window and a pool of brick slots, so that what leaves the window can be kept and put back.
 *
 * Like include/ovn_hip_deskew.h these entry points are ADDITIONS: the tables that pin ovn_hip.h (tests/test_abi.py,
 * tests/test_engine_calls_host.py) and the deskew extension (tests/test_deskew_host.py) stay as they are, so the calls are declared
 * here, bound from `_lib.STORE_SIGNATURES` and guarded by tests/test_tsdf_store_host.py.  OVN_ABI_VERSION does not change.
 *
 * The conventions are those of ovn_hip.h: "dev" pointers are device memory owned by the caller; `stream` is a hipStream_t passed as
 * void* (NULL = the legacy default stream) and a call only ENQUEUES work on it; the context's device is selected for the call's
 * duration and the caller's current device restored; 0 = success, else an error whose message ovn_last_error() returns.  `ctx` comes
 * first and `stream` second; tests/test_gpu_tsdf_store_stream.py runs the calls on a non-default stream.
 *
 * The window arguments tsdf_dev, weight_dev, nx, ny, nz, base have the meaning and the refusals of ovn_tsdf_window_*: (nz,ny,nx) f32
 * ring storage, sample I of an axis in slot I mod n, every dimension a multiple of 8 and >= 16, every component of base a multiple of
 * 8, every lattice index within 2^20.  Here both arrays must also be 16-byte aligned.  A BRICK (bi, bj, bk) is the 8 x 8 x 8 lattice
 * samples 8 bi .. 8 bi + 7, 8 bj .. 8 bj + 7, 8 bk .. 8 bk + 7.  Because n and base are multiples of 8, a window holds whole bricks
 * only, a brick's eight slots on an axis are consecutive (no brick straddles a ring seam), and its eight x samples are one aligned
 * 32-byte run of a row.
 */
#ifndef OVN_HIP_TSDF_STORE_H
#define OVN_HIP_TSDF_STORE_H

#include "ovn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1024 f32 words per pool slot: the brick's 512 tsdf words, then its 512 weight words, each z, y, x with x fastest */
#define OVN_TSDF_BRICK_WORDS 1024

/* ovn_tsdf_window_brick_flags: which bricks of a box of the window hold anything (csrc/tsdf_store.hip).
 *   box_lo, box_hi  3 int32 each (host): the box in lattice BRICK coordinates (sample index / 8), hi exclusive; lo <= hi, and the box
 *                   lies inside the window: 8 lo >= base and 8 hi <= base + n on every axis
 *   flags_dev       (hi_z - lo_z) (hi_y - lo_y) (hi_x - lo_x) uint8, z-major, then y, then x: 1 iff some sample of the brick differs in
 *                   its WORDS from (tsdf 1.0f, weight 0.0f) -- bit patterns are compared (0x3f800000 and 0x00000000), so a sample with
 *                   weight 0 and tsdf != 1 counts, and so does a weight of -0.0f -- else 0.  Every byte of the box is written
 * One wave reduces one brick: each lane reads four 16-byte pieces, a ballot joins them; no LDS, no atomics.  An empty box is a no-op.
 * OVN_ERR_ARG, before any launch: a NULL ctx, a NULL array or box; a window ovn_tsdf_window_* refuses; an array that is not 16-byte
 * aligned; a box with lo > hi or outside the window; a NULL flags_dev for a box that is not empty. */
int ovn_tsdf_window_brick_flags(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                                const int32_t* base, const int32_t* box_lo, const int32_t* box_hi, uint8_t* flags_dev);

/* ovn_tsdf_window_page_out: each listed brick copied from the ring into its pool slot; the window is not written.
 *   n           the number of bricks, >= 0; 0 is a no-op without a launch
 *   bricks_dev  (n,3) int32: the lattice brick coordinates (bi, bj, bk), inside the window
 *   slots_dev   (n) int32: the pool slot of each, >= 0
 *   pool_dev    f32, OVN_TSDF_BRICK_WORDS per slot, 16-byte aligned; slot s starts at word 1024 s (64-bit offsets)
 * The lists are the host's, unique by construction and trusted like other device index lists -- but a brick outside the window or a
 * negative slot is skipped, not followed.  One workgroup of 256 threads per brick, one 16-byte load and one 16-byte store per thread;
 * the pool side is 4 KB contiguous, the ring side 128 aligned runs of 32 bytes.  No LDS, no atomics, no scratch of the context.
 * OVN_ERR_ARG, before any launch: a NULL ctx; n < 0; a NULL array; a window ovn_tsdf_window_* refuses; and for n > 0 a NULL list or
 * pool, or tsdf_dev, weight_dev or pool_dev not 16-byte aligned. */
int ovn_tsdf_window_page_out(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                             const int32_t* base, int n, const int32_t* bricks_dev, const int32_t* slots_dev, float* pool_dev);

/* ovn_tsdf_window_page_in: the reverse copy, pool slot -> ring; the pool is not written.  Arguments and refusals as for
 * ovn_tsdf_window_page_out. */
int ovn_tsdf_window_page_in(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const int32_t* base,
                            int n, const int32_t* bricks_dev, const int32_t* slots_dev, const float* pool_dev);

#ifdef __cplusplus
}
#endif

#endif /* OVN_HIP_TSDF_STORE_H */
