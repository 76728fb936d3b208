/*
 * ovn_hip.h -- C ABI of libovn_hip.so, the MI355X (gfx950) OverlapNet inference hot path.
 *
 * The reference (PRBonn/OverlapNet) has no FFI layer of its own: its hot path is reached through the
 * Python class `Infer` (src/two_heads/infer.py:22) which hands everything to Keras/TensorFlow.  These
 * entry points are what a binding for that path has to reach; each one names the reference code it
 * replaces.  The Python host (`overlapnet_amd/infer.py`) calls them through ctypes.
 *
 * Conventions
 *   - every pointer marked "dev" is a DEVICE pointer (HIP memory owned by the caller, e.g. a torch
 *     tensor's data_ptr()); the library never takes ownership and never frees caller memory;
 *   - all tensors are float32, channels-last (NHWC), densely packed;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); every call only
 *     ENQUEUES work on it, nothing synchronises unless stated.  One exception: a context owns ONE scratch
 *     block that grows on demand; a call that needs more than any earlier call synchronises `stream`
 *     once to re-allocate it.  All calls on one context must therefore be issued on one stream at a time
 *     (two streams would race on the scratch).  A head call may internally fork onto context-owned side
 *     streams; it joins them back into `stream` before it returns (events, no host synchronisation);
 *   - every entry point selects the context's device for its own duration and restores the caller's
 *     current HIP device before it returns;
 *   - return value 0 = success, non-zero = error, message via ovn_last_error() (thread-local);
 *   - one context per GPU per process; calls on one context are not re-entrant (the reference object
 *     is not thread-safe either: mutable feature cache, infer.py:114,185).
 */
#ifndef OVN_HIP_H
#define OVN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ovn_ctx ovn_ctx;

#define OVN_OK 0
#define OVN_ERR_ARG 1      /* bad argument / unsupported shape */
#define OVN_ERR_HIP 2      /* HIP runtime error                */
#define OVN_ERR_STATE 3    /* call order (weights missing ...)  */

/* ABI version of this header; bumped on any signature change. */
#define OVN_ABI_VERSION 11
int ovn_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* ovn_last_error(void);

/* Create / destroy a context bound to HIP device `device_id` for leg inputs of in_h x in_w x in_c
 * (64 x 900 x C in the reference, infer.py:76-82).  Replaces the model construction of
 * Infer.__init__ (infer.py:86-111). */
int ovn_create(int device_id, int in_h, int in_w, int in_c, ovn_ctx** out);
int ovn_destroy(ovn_ctx* ctx);

/* Register one convolution layer of the leg, in network order (generateNet.py:161-214: s_conv1 ...
 * s_conv10).  kernel_dev: Keras layout (kh, kw, cin, cout); bias_dev: (cout).  The library keeps its
 * own re-tiled copy (MFMA fragment order), so the caller may release its buffers after the call
 * returns (the call synchronises `stream`).  All leg layers are valid-padded + bias + ReLU.
 * Geometry: any kh, kw, cin, stride_h, stride_w >= 1 and any cout that is a multiple of 16; cin must be
 * the cout of the layer registered before (the context's in_c for the first).  Anything else returns
 * OVN_ERR_ARG and leaves the context as it was: a valid layer may follow.
 * One rule depends on the input size, which is only known per call: in leg precision f16x3 (the default,
 * ovn_set_leg_precision) a layer that none of the shape-specialised leg kernels takes -- every layer but
 * the reference's s_conv1 with strides (2, 2) at in_c = 4 and s_conv2 ... s_conv10 -- runs a general
 * kernel whose tiles need at least 128 output positions (oh * ow) per image.  For the context's own
 * input size the rule is applied where everything is known: ovn_finalize in leg precision f16x3, and
 * ovn_set_leg_precision(ctx, 1) on a finalized context, return OVN_ERR_ARG "layer <name>: fewer than 128
 * output positions per image" (set precision f32 before ovn_finalize to run such a leg in fp32), so
 * ovn_leg never meets it.  ovn_debug_conv takes its input size per call and returns the same error
 * before launching the layer, writing nothing to the output.  Leg precision f32, the training forward
 * and the backward pass have no such limit.  Every leg the reference's `strides_layer1` can produce for
 * a feature volume of 1 x W, W >= 45, gives its first layer more positions than that.
 * Replaces `leg.load_weights(file, by_name=True)` (infer.py:119). */
int ovn_add_leg_layer(ovn_ctx* ctx, const char* name, const float* kernel_dev, const float* bias_dev,
                      int kh, int kw, int cin, int cout, int stride_h, int stride_w, void* stream);

/* Register the Delta-head weights (generateNet.py:96-114): c_conv1 (1,15,128,64) linear,
 * c_conv2 (15,1,64,128) ReLU, c_conv3 (3,3,128,256) ReLU, overlap_output Dense (123904,1) sigmoid.
 * Same ownership rule as above.  Replaces `head.load_weights(...)` (infer.py:120). */
int ovn_set_head_weights(ovn_ctx* ctx, const float* c1_kernel_dev, const float* c1_bias_dev,
                         const float* c2_kernel_dev, const float* c2_bias_dev,
                         const float* c3_kernel_dev, const float* c3_bias_dev,
                         const float* dense_kernel_dev, const float* dense_bias_dev, void* stream);

/* Head geometry: `conv1NetworkHead_conv1size` of the reference's network.yml (generateNet.py:88-99: the 1 x s / s x 1 kernels and
 * strides of c_conv1 / c_conv2; default 15, which the shipped configuration uses).  Call BEFORE ovn_set_head_weights when the
 * model was built with another value: c_conv1 is then (1, s, 128, 64), c_conv2 (s, 1, 64, 128) and the Dense kernel has
 * (feat_w // s - 2)^2 * 256 inputs (feat_w = 360 before ovn_finalize).  The MFMA-tiled Delta kernels (both arithmetic modes) serve s = 15; any other s runs a general fp32
 * path (DeltaLayer + c_conv1 as plain FMAs without materialising the difference tensor, c_conv2 / c_conv3 through the generic fp32
 * convolution) -- correct to the same tolerance, an order of magnitude slower, no Delta cache. */
int ovn_set_head_geometry(ovn_ctx* ctx, int conv1size);

/* Validate the registered leg chain: output must be 1 x feat_w x 128 with OVN_FEAT_W_MIN <= feat_w <= OVN_FEAT_W_MAX
 * (1 x 360 x 128 in the reference's shipped configuration; the reference derives the width from `inputShape`, `strides_layer1`
 * and `additional_unsymmetric_layer3a`, generateNet.py:143-146).  Writes the leg output width to *feat_w.
 *
 * Width rule.  Every feature volume a context reads or writes is feat_w x 128 floats, corr vectors are feat_w floats, and the Delta
 * head has G = feat_w // conv1size column groups (at least 3) and a Dense kernel of (G - 2)^2 * 256 inputs.  At feat_w = 360 every
 * route of this header is available.  At any other width the heads run exact fp32 on the fp32 MFMA in every head precision mode
 * (ovn_set_head_precision is accepted and has no effect there: the tuned split-operand kernels are tiled to 24 groups of 15 and to
 * the 360-point DFT) unless ovn_set_head_width_split asks for the f16x3 Delta head there, and the 360-only entry points ovn_spectrum, ovn_corr_head_spectral, ovn_heads_spectral and ovn_delta_cache
 * return OVN_ERR_ARG.  If ovn_set_head_weights ran first, finalize also requires feat_w // conv1size to match the Dense kernel
 * registered there. */
#define OVN_FEAT_W_MIN 45
#define OVN_FEAT_W_MAX 512
int ovn_finalize(ovn_ctx* ctx, int* feat_w);

/* Leg: images_dev (n, in_h, in_w, in_c) -> features_dev (n, feat_w, 128).
 * Replaces `leg.predict_generator` in Infer.create_feature_volumes (infer.py:262-265).
 * A scan's feature volume depends on that scan alone: every call size runs the same kernels, and the power-of-two scales of the
 * f16x3 arithmetic are taken per scan (per strip / tile inside the fused first two layers and the fused tail) -- the same scan computed alone,
 * inside any batch, at any position and next to any other scans gives the same bits (the reference's `predict_generator` results
 * do not depend on batch composition either, infer.py:262-265).  Calls of more than 1024 scans are processed in equal slices of at
 * most 1024 (scratch: 2 x slice x 770 KB at in_c = 4, i.e. up to 1.6 GB, see ovn_workspace_bytes). */
int ovn_leg(ovn_ctx* ctx, const float* images_dev, int64_t n, float* features_dev, void* stream);

/* Both heads on n pairs.  Pair p uses l = feats_l_dev[lidx[p]] and r = feats_r_dev[ridx[p]]
 * (each feature volume feat_w x 128 floats); lidx_dev == NULL means lidx[p] = p, ridx_dev == NULL means
 * ridx[p] = 0 (the 1-vs-N sweep of Infer.infer_multiple, infer.py:188-190: l = candidate, r = query).
 * Outputs (any may be NULL except overlap/yaw):
 *   overlap_dev (n) f32  = sigmoid(logit)            (generateNet.py:114)
 *   yaw_dev     (n) i32  = 180 - argmax_k corr[k]    (infer.py:158; first maximum wins)
 *   logit_dev   (n) f32  pre-sigmoid value
 *   corr_dev    (n, feat_w) f32 orientation_output   (generateNet.py:352)
 * Replaces `head.predict_generator` + post-processing (infer.py:155-158,194-198,229-233) and the pair
 * gather of ImagePairOverlapSequenceFeatureVolume.__getitem__ (:43-47).
 * What a pair's bits depend on (f16x3 arithmetic): its two volumes and the left volume's SLOT in feats_l_dev modulo 32 (lidx[p],
 * or p without an index list) -- not on n, on the chunking of the sweep, on the order of the index list or on the workgroup
 * decomposition the library picks for small n.  A shard of a pool that starts at a slot which is a multiple of 32 therefore
 * reproduces the unsharded sweep bit for bit (overlapnet_amd/distributed.py: shard_bounds(align = 32), frame_slot).  The fp32 mode
 * has one fixed summation order: its bits do not depend on the slot either. */
int ovn_heads(ovn_ctx* ctx, const float* feats_l_dev, const int32_t* lidx_dev, const float* feats_r_dev,
              const int32_t* ridx_dev, int64_t n, float* overlap_dev, int32_t* yaw_dev, float* logit_dev,
              float* corr_dev, void* stream);

/* Delta (overlap) head alone (generateNet.py:64-116): overlap (n) f32, optional logit (n); indexing as ovn_heads.
 * Used together with ovn_corr_head_spectral when candidate spectra are cached. */
int ovn_delta_head(ovn_ctx* ctx, const float* feats_l_dev, const int32_t* lidx_dev, const float* feats_r_dev,
                   const int32_t* ridx_dev, int64_t n, float* overlap_dev, float* logit_dev, void* stream);

/* Correlation (yaw) head alone (NormalizedCorrelation2D.py:43-109 with the normalisation of ovn_set_corr_normalization, 'none' by
 * default); same indexing convention as ovn_heads.  Both volumes are normalised on the fly. */
int ovn_corr_head(ovn_ctx* ctx, const float* feats_l_dev, const int32_t* lidx_dev, const float* feats_r_dev,
                  const int32_t* ridx_dev, int64_t n, int32_t* yaw_dev, float* corr_dev, void* stream);

/* Spectral form of the correlation head (same result as ovn_corr_head up to fp32 rounding, HBM-bound):
 * ovn_spectrum turns feature volumes (n, 360, 128) into cached spectra (n, 128, 368) -- per channel the 181
 * non-redundant DFT bins, real parts at [0..180], imaginary parts at [184..364], zero padding elsewhere;
 * ovn_corr_head_spectral evaluates corr = IDFT( sum_c L^ conj(R^) ) shifted by W/2 and the argmax for n pairs
 * (l = spec_l[lidx[p]], r = spec_r[ridx[p]]; NULL index arrays as in ovn_heads).  yaw (n) int32, corr (n,360) or NULL.
 * Replaces NormalizedCorrelation2D.call (NormalizedCorrelation2D.py:43-109) + infer.py:158 for 1-vs-N sweeps. */
int ovn_spectrum(ovn_ctx* ctx, const float* feats_dev, int64_t n, float* spectra_dev, void* stream);
int ovn_corr_head_spectral(ovn_ctx* ctx, const float* spec_l_dev, const int32_t* lidx_dev, const float* spec_r_dev,
                           const int32_t* ridx_dev, int64_t n, int32_t* yaw_dev, float* corr_dev, void* stream);

/* Delta cache: everything of a pair's Delta-head preparation that depends on the LEFT volume (the candidate of a sweep) alone --
 * its feature volume re-written as the packed hi/lo fp16 words the contraction kernel streams (at the candidate's own power-of-two
 * scale; channel-major [128][360], so that a sweep fetches only the channels alive in its query: ovn_set_head_compaction), its linear term pushed through c_conv2 (TT + b2) and its value range.  OVN_DELTA_CACHE_ELEMS floats (196,864 B) per
 * volume, cached next to the feature volume and the spectrum (the reference caches per-candidate state too: infer.py:184-185).
 * A row is used by ovn_heads_spectral for a pair whenever neither volume has a negative value and the query's largest value is
 * below the candidate's next power of two; every other pair is prepared in scratch as without a cache -- same bits either way.
 * Valid for the head weights registered when it was built (f16x3 head mode; the fp32 mode ignores it). */
#define OVN_DELTA_CACHE_ELEMS 49216
int ovn_delta_cache(ovn_ctx* ctx, const float* feats_dev, int64_t n, float* cache_dev, void* stream);

/* Fitting the Delta head on frozen legs (the reference's `360OutputkLegsFixed` model, training.py): the gradient of
 *   L = scale / n * sum_p loss(y_p, t_p),  y_p = the overlap of pair p, t_p = target_dev[p]
 * with respect to the eight head tensors as registered by ovn_set_head_weights.  Indexing as ovn_heads (lidx NULL: p, ridx NULL: 0).
 *   loss 0   the reference's my_sigmoid_loss (training.py:71-83): sigmoid(24 |y - t| - 6), d/dy = 24 l (1 - l) sign(y - t), sign(0) = 0
 *   loss 1   squared error (y - t)^2
 * ovn_head_param_sizes: elements of c_conv1 kernel, c_conv1 bias, c_conv2 kernel, c_conv2 bias, c_conv3 kernel, c_conv3 bias, Dense
 * kernel, Dense bias for the context's geometry (s = conv1size, W = feat_w, G = W // s): 128 s 64, 64, s 64 128, 128, 3 3 128 256, 256,
 * (G - 2)^2 256, 1.
 *   grad_dev     the eight gradients in that order, concatenated, each in its Keras layout
 *   loss_dev     1 float: L
 *   overlap_dev  (n) or NULL: y
 *   o2_dev, o3_dev   (n, G, G, 128), (n, G - 2, G - 2, 256) or NULL: the c_conv2 / c_conv3 activations of the forward pass
 * The forward pass has fp32 operands and keeps every stage output in fp32, at any conv1size and width; the sums of a stage are
 * carried in fp64 and rounded once (the gradient is sensitive to the logit's rounding error), so overlap_dev
 * may differ from ovn_heads' in the last bits.  ovn_set_head_precision does not affect this call.  ReLU'(0) = 0, the masks come from the stored activations.  A c_conv1
 * kernel registered negated (DeltaLayer negateDiffs) gets the gradient of that negated kernel.
 * Deterministic: no floating-point atomics; partial sums per block of OVN_GRAD_PAIR_BLOCK consecutive pairs are added in pair-block
 * order, so the same call gives the same bits, whatever chunks of pairs the workspace forces (ovn_set_head_pipeline's chunk_pairs
 * bounds them; chunks are whole pair blocks).  Workspace: about three times the forward's stage outputs per pair of a chunk
 * (6.3 MB at 360 / 15) plus one set of gradients per pair block.  Under ovn_profile_begin the kernels report as classes 2 (forward),
 * 4 (loss, Dense gradients), 3 (c_conv3 gradients), 9 (c_conv2 gradients), 8 (c_conv1 gradients).
 * OVN_ERR_ARG before any launch: NULL ctx / feats / target / grad / loss pointer, n < 1, another `loss`, a non-finite scale;
 * OVN_ERR_STATE: head weights not registered. */
#define OVN_GRAD_PAIR_BLOCK 4
int ovn_head_param_sizes(ovn_ctx* ctx, int64_t* sizes8);
int ovn_delta_head_grad(ovn_ctx* ctx, const float* feats_l_dev, const int32_t* lidx_dev, const float* feats_r_dev,
                        const int32_t* ridx_dev, int64_t n, const float* target_dev, int loss, float scale, float* grad_dev,
                        float* loss_dev, float* overlap_dev, float* o2_dev, float* o3_dev, void* stream);

/* Both heads' losses differentiated down to the leg outputs (the feature volumes): what a leg trainer needs from the heads.
 *   L_ov  = overlap_scale / n * sum_p loss(y_p, t_p)                       exactly the loss of ovn_delta_head_grad (same `loss` codes)
 *   L_yaw = yaw_scale / (n W) * sum_p sum_{k < W} wce(z_p[k], q_p[k])      the reference's my_entropy (training.py:86-92):
 *           z_p[k] = sum_{j < W, c < 128} l_p[(k + j + W / 2) mod W, c] r_p[j, c]   (NormalizedCorrelation2D 'none' + RangePadding2D),
 *           q_p[k] = 1 where k == yaw_bin_dev[p] and t_p > min_overlap_for_angle, else 0 (a pair at or below the threshold has q = 0
 *           and still contributes), wce = weighted_cross_entropy_with_logits with pos_weight = W:
 *           (1 - q) z + (1 + (W - 1) q) (log1p(exp(-|z|)) + max(-z, 0)).
 *   dfeat_l_dev, dfeat_r_dev   (n, W, 128): row p = d (L_ov + L_yaw) / d (the left / right volume pair p read).  Per PAIR: rows that
 *                    address the same pool entry are not summed here (no atomics, no knowledge of the pool).  The overlap part reaches
 *                    rows < s (W // s) only; sgn(0) = 0 in d|l - r|.
 *   head_grad_dev    NULL, or the eight head gradients: the bits ovn_delta_head_grad returns for scale = overlap_scale
 *   loss_dev         2 floats: L_ov, L_yaw
 *   overlap_dev      (n) or NULL: y, the bits of ovn_delta_head_grad;  corr_dev  (n, W) or NULL: z as defined above, always the
 *                    un-normalised logits, whatever ovn_set_corr_normalization holds (also when the yaw part is off); NULL with
 *                    the yaw part off skips the correlation altogether
 * yaw_bin_dev == NULL or yaw_scale == 0: no yaw part, L_yaw = 0.  overlap_scale == 0: the overlap backward is skipped, its share is
 * exact zeros, head_grad_dev (if given) is zero-filled, L_ov = 0.  A bin outside [0, W) gives its pair q = 0; it is compared, never
 * used as an index.  Only correlation normalisation mode 0 ('none', the mode generateCorrelationHead builds) is differentiated.
 * The forward is ovn_delta_head_grad's (fp64 sums, rounded once); so are z, the scalar chain z -> loss, dL/dz and the yaw gradients.
 * The Delta data gradient forms E[i, j, c] = sum_o dO1[i, j // s, o] W1[j % s, c, o] tile by tile on the fp32 matrix cores, with the
 * sign of l - r applied in registers; E is never stored.  fp32 sums run over at most one column group, the groups join in fp64.
 * Deterministic: no floating-point atomics; the same bits twice and in any chunking (as ovn_delta_head_grad); both loss sums
 * join in pair-block order.  ovn_set_head_pipeline's chunk_pairs cuts the overlap part only; the yaw part runs in fixed chunks of
 * 4096 pairs (whole pair blocks, so the bits do not depend on it).  Workspace: ovn_delta_head_grad's, then 12 W bytes per pair (of
 * at most 4096) for the yaw part, which chunk_pairs does not limit.  Under
 * ovn_profile_begin the Delta data gradient reports as class 8, the correlation forward / yaw loss / yaw gradients as class 1.
 * OVN_ERR_ARG before any launch: NULL ctx / feats / target / dfeat / loss pointer, n < 1, another `loss`, a non-finite scale or
 * threshold; OVN_ERR_STATE: head weights not registered, or the yaw part requested under a correlation normalisation other than 0. */
int ovn_heads_feature_grad(ovn_ctx* ctx, const float* feats_l_dev, const int32_t* lidx_dev, const float* feats_r_dev,
                           const int32_t* ridx_dev, int64_t n, const float* overlap_target_dev, const int32_t* yaw_bin_dev, int loss,
                           float overlap_scale, float yaw_scale, float min_overlap_for_angle, float* dfeat_l_dev, float* dfeat_r_dev,
                           float* head_grad_dev, float* loss_dev, float* overlap_dev, float* corr_dev, void* stream);

/* Training the legs (the reference's default: training.py trains the whole Siamese network): the leg's forward with every layer
 * output kept, and its backward.  Together with ovn_heads_feature_grad this is the gradient of both losses with respect to all
 * 2 x layers leg tensors.
 *   ovn_leg_layer_count        *layers = number of registered leg layers
 *   ovn_leg_param_sizes        sizes[2 li], sizes[2 li + 1] = elements of layer li's kernel (kh, kw, cin, cout: Keras layout) and bias
 *   ovn_leg_activation_sizes   sizes[li] = elements per scan of layer li's output (oh, ow, cout) for the context's input geometry
 * ovn_leg_forward_train: images_dev (n, in_h, in_w, in_c) -> acts_dev, layer-major: block li is (n, oh_li, ow_li, cout_li), all n
 *   scans of a layer together; the last block is the feature volumes (n, feat_w, 128).  Exact fp32 (the fp32 MFMA convolution of leg
 *   precision 0, layer by layer), whatever ovn_set_leg_precision holds: the last block has the bits ovn_leg gives in precision 0.
 * ovn_leg_backward: dfeat_dev (n, feat_w, 128) = dL/d(feature volume of scan i), already summed over the pairs that read it;
 *   grad_dev = the 2 x layers gradients in the order of ovn_leg_param_sizes, concatenated, each summed over the n scans.
 *   ReLU'(0) = 0, the masks come from acts_dev.  The input images get no gradient (nothing trains upstream), so the data gradient
 *   stops at the input of the second layer.  slice_scans: 0 = the library's choice (32); otherwise the scans are processed in slices
 *   of at most that many, rounded down to whole scan blocks (at least one).
 *   Sums: an fp32 MFMA accumulator runs over at most 256 terms; everything above that joins in fp64 and is rounded once.
 *   Deterministic: no floating-point atomics; partial sums are cut inside blocks of OVN_LEG_GRAD_SCAN_BLOCK consecutive scans and
 *   added in (scan block, piece) order, so the same call gives the same bits twice, and the same bits for every slice_scans.
 *   Workspace: two buffers of the largest activation per scan of a slice, the fp64 sums (8 bytes per weight) and the partials of
 *   one layer (a slice of 32 scans of 64 x 900 x 4: about 200 MB).  The kernels report as class 0 under ovn_profile_begin.
 * ovn_set_leg_layer_weights: replaces the weights of leg layer `layer` in a FINALIZED context (ovn_add_leg_layer keeps refusing
 *   calls after ovn_finalize) and rebuilds every copy derived from them; afterwards ovn_leg in every precision mode gives the bits
 *   of a fresh context loaded with the new weights.  Synchronises `stream`.  Cached feature volumes, spectra and Delta cache rows
 *   computed by the old weights are stale.
 * ovn_debug_conv_grad (test hook, companion of ovn_debug_conv): the three gradients of leg layer `layer` alone on an arbitrary
 *   input in_dev (nb, h, w, cin) with its stored output out_dev (nb, oh, ow, cout) and dout_dev = dL/d(out): din_dev (nb, h, w, cin),
 *   dkernel_dev, dbias_dev; any of the three may be NULL.  din_dev is available for every layer: a layer whose cin is not a multiple
 *   of 16 (the first one) runs a plain fp64 kernel instead of the MFMA one.
 * OVN_ERR_ARG before any launch: NULL ctx / buffer, n (nb) < 1, slice_scans < 0, a bad layer index, an input smaller than the kernel;
 * OVN_ERR_STATE: context not finalized (ovn_leg_activation_sizes, ovn_leg_forward_train, ovn_leg_backward, ovn_set_leg_layer_weights). */
#define OVN_LEG_GRAD_SCAN_BLOCK 4
int ovn_leg_layer_count(ovn_ctx* ctx, int* layers);
int ovn_leg_param_sizes(ovn_ctx* ctx, int64_t* sizes);
int ovn_leg_activation_sizes(ovn_ctx* ctx, int64_t* sizes);
int ovn_leg_forward_train(ovn_ctx* ctx, const float* images_dev, int64_t n, float* acts_dev, void* stream);
int ovn_leg_backward(ovn_ctx* ctx, const float* images_dev, const float* acts_dev, int64_t n, const float* dfeat_dev, float* grad_dev,
                     int64_t slice_scans, void* stream);
int ovn_set_leg_layer_weights(ovn_ctx* ctx, int layer, const float* kernel_dev, const float* bias_dev, void* stream);
int ovn_debug_conv_grad(ovn_ctx* ctx, int layer, const float* in_dev, const float* out_dev, const float* dout_dev, int nb, int h, int w,
                        float* din_dev, float* dkernel_dev, float* dbias_dev, void* stream);

/* Data-parallel training: the gradients of `world` ranks reduced and Keras 2.1.5's Adagrad applied, one kernel (grad_reduce.hip).
 *   grads_dev         (world, stride) float32: row r holds the flat gradient of rank r in its first `count` elements
 *   rank_weight_host  world doubles on the HOST: n_r / n, the share of the global batch rank r held
 *   params_dev, accum_dev   (count) each, updated in place; both NULL: the call only reduces
 *   grad_out_dev      (count) or NULL: the reduced gradient
 * For every i < count, each operation one correctly rounded IEEE operation (nothing fused, fp32 denormals kept):
 *   s = 0.0 (fp64); for r = 0 .. world - 1 in this order, rows with weight 0.0 skipped and NOT READ:  s = s + w[r] * (double)G[r][i]
 *   g = (float)s;  grad_out[i] = g;  a = accum[i] + g * g;  accum[i] = a;  params[i] = params[i] - (lr * g) / (sqrtf(a) + eps)
 * No atomics, a fixed order: the same bits on every call and every rank.  Buffers that are all 16-byte aligned are walked with
 * 16-byte accesses; any other alignment is served element by element.  Reports as class 0 under ovn_profile_begin.
 * OVN_ERR_ARG before any launch: NULL ctx / grads / weights, world outside 1..OVN_GRAD_REDUCE_MAX_WORLD, count < 1, stride < count
 * or not a multiple of 4, exactly one of params / accum NULL, all three outputs NULL, a non-finite lr or eps, eps < 0, a weight that
 * is negative or not finite, all weights zero. */
#define OVN_GRAD_REDUCE_MAX_WORLD 64
int ovn_grad_reduce_adagrad(ovn_ctx* ctx, const float* grads_dev, int world, int64_t stride, const double* rank_weight_host,
                            int64_t count, float* params_dev, float* accum_dev, float lr, float eps, float* grad_out_dev, void* stream);

/* Normalisation of the correlation head's inputs, NormalizedCorrelation2D(normalize=...) (NormalizedCorrelation2D.py:23-73):
 *   0 none (default; what generateCorrelationHead builds, generateNet.py:343), 1 euclidean (the layer's own default:
 *   x / sqrt(max(sum x^2, 1e-12))), 2 scaling ((x - min) / (max - min + 1e-6)), 3 standardization (y = x - mean + 1e-5,
 *   y / sqrt(max(sum y^2, 1e-12))), each per (volume, channel) over the 360 columns; any other value: OVN_ERR_ARG.
 * Statistics in fp64 in one fixed order, each element evaluated in fp64 and rounded once to fp32: a volume's normalised values do not
 * depend on the call, the batch or the pair.  The Delta head reads the raw volumes in every mode (so do Delta cache rows).
 *   ovn_corr_head, ovn_heads (no spectra)   normalise both volumes on the fly; corr_dev is the normalised correlation.
 *   ovn_spectrum                            writes the spectrum of the NORMALISED volume: a cached spectrum is valid for the mode
 *                                           it was built under (the same rule as Delta cache rows and head weights).
 *   ovn_corr_head_spectral, ovn_heads_spectral   consume such spectra unchanged.
 * Mode 0 runs the kernels of ABI 7 unchanged, with the same launches and bits. */
int ovn_set_corr_normalization(ovn_ctx* ctx, int mode);
int ovn_get_corr_normalization(ovn_ctx* ctx, int* mode);

/* Both heads of a sweep whose candidates have their spectra (and optionally their Delta cache rows, dcache_l_dev, may be NULL) cached
 * next to their feature volumes: what `Infer.infer_multiple` runs per query.  Same outputs and indexing as ovn_heads (one index
 * array addresses the feature, spectrum and Delta-cache pools alike); the Delta head reads the feature volumes / cache rows, the yaw
 * head the spectra (ONE launch for the whole sweep).  The Delta cache is used in the 1-vs-N form (ridx_dev == NULL).  With
 * ovn_set_head_pipeline the call can fork the independent kernel chains over context-owned side streams; it joins them back into
 * `stream` with events before it returns: to the caller everything is ordered as if enqueued on `stream`.
 * Replaces `head.predict_generator` + post-processing for 1-vs-N sweeps (infer.py:188-198). */
int ovn_heads_spectral(ovn_ctx* ctx, const float* feats_l_dev, const float* spec_l_dev, const float* dcache_l_dev,
                       const int32_t* lidx_dev, const float* feats_r_dev, const float* spec_r_dev, const int32_t* ridx_dev, int64_t n,
                       float* overlap_dev, int32_t* yaw_dev, float* logit_dev, float* corr_dev, void* stream);

/* Both heads on a batch of B loop-closure queries, each with its own candidate list (a SEGMENT), in one call: the offline form of
 * B calls of ovn_heads_spectral (or ovn_heads, without spectra) in their 1-vs-N form.  The batch is stored like a CSR matrix:
 *   seg_offsets  HOST array, B + 1 int64: seg_offsets[0] == 0, non-decreasing, seg_offsets[B] == n; segment b is the pairs
 *                [seg_offsets[b], seg_offsets[b + 1]) (empty segments are allowed)
 *   query_idx    HOST array, B int32 >= 0: segment b's query is feats_q_dev[query_idx[b]] (spec_q_dev alike)
 *   cand_idx_dev DEVICE array, n int32: pair p's candidate is feats_pool_dev[cand_idx[p]] (spec_pool_dev, dcache_pool_dev alike)
 * Pair p of segment b = (left = pool[cand_idx[p]], right = queries[query_idx[b]]): candidate -> head-left, query -> head-right, the
 * orientation of Infer.infer_multiple.  The two pools may be the same tensors.  spec_pool_dev / spec_q_dev: both or neither (360
 * columns only); dcache_pool_dev may be NULL.  Outputs are flat (n), in pair order, as in ovn_heads.
 * Contract: pair p gets the bits ovn_heads_spectral (ovn_heads without spectra) returns for it when segment b is run alone in its
 * 1-vs-N form -- lidx = cand_idx[seg_offsets[b] ..], ridx NULL, feats_r = the query -- with the same pools, settings and precision mode.
 * Route: in the f16x3 mode at W = 360 with conv1size 15 and compaction on, the batch runs in passes of at most the head chunk
 * (ovn_set_head_pipeline) and OVN_SEG_PASS_MAX segments.  A pass computes each segment's query state once, in one launch per kernel
 * for all its segments (A2, the query block, the live-channel list, the W1 fragments gathered for it); the prepare and contraction
 * kernels find a pair's through its segment.  All segments of a pass share one kernel chain.  Every other mode and geometry, and
 * f16x3 with compaction off (its 1-vs-N walk is the indexed walk), runs one indexed pass over all pairs.  The per-pair query and
 * segment indices come from one small kernel over the staged table.
 * Argument errors return OVN_ERR_ARG before any launch: B outside [0, 2^31), bad offsets, n != seg_offsets[B], a negative
 * query_idx, spec_* given alone, misaligned pointers (4 bytes; dcache_pool_dev 16).  The library does not range-check the device
 * array cand_idx_dev or query_idx's upper end against the pools (as with lidx / ridx of ovn_heads): the caller does.
 * n == 0 is a no-op.  Workspace (ovn_workspace_bytes): that of a head call over one chunk, plus 2 MB of query state per segment of a
 * pass (at most OVN_SEG_PASS_MAX x 2 MB), plus a context-owned table of 8 (B + 1) + 4 B + 8 n bytes on the device and 8 (B + 1) + 4 B
 * in pinned host memory.  The host arrays may be reused as soon as the call returns.  Successive segmented calls may use different
 * streams: each waits for the previous one's kernels before it rewrites the table.  The table is staged through ONE pinned buffer:
 * a segmented call (this one or ovn_top_k_segments) made while the previous one's table copy is still pending on its stream waits on
 * the host for that copy.  A segmented call that follows a drained stream only enqueues.  (The wait guards the reuse of the staging
 * buffer, it returns nothing to the host: a second staging buffer would remove it.  Kept, because the table is a few KB whose copy
 * is over long before a caller has post-processed one batch and assembled the next.) */
int ovn_heads_segments(ovn_ctx* ctx, const float* feats_pool_dev, const float* spec_pool_dev, const float* dcache_pool_dev,
                       const int32_t* cand_idx_dev, const float* feats_q_dev, const float* spec_q_dev, const int32_t* query_idx,
                       const int64_t* seg_offsets, int64_t B, int64_t n, float* overlap_dev, int32_t* yaw_dev, float* logit_dev,
                       float* corr_dev, void* stream);
#define OVN_SEG_PASS_MAX 128

/* Launch structure of the head calls (the reference's counterpart is `batch_size`, network.yml:41, which sets how many pairs one
 * predict step materialises):
 *   chunk_pairs          pairs per pass over the context's scratch (default 1024).  The f16x3 Delta path needs 2.9 MB of scratch
 *                        per pair of a chunk (packed volumes, linear terms, the c_conv1 rows between its two kernels):
 *                        ovn_workspace_bytes ~ 3.3 GB at the default; a sweep longer than a chunk is processed in several passes;
 *   sub_chunk_pairs      0 = none; otherwise every chunk is cut into sub-chunks of this many pairs whose kernel chains
 *                        alternate between `streams` (1 or 2) streams -- the prepare / c_conv2 / c_conv3 kernels of one sub-chunk
 *                        then run beside the contraction kernel of the next;
 *   yaw_on_side_stream   ovn_heads_spectral runs its yaw kernel on a side stream.
 * Defaults: 1024, 0, 1, 0 -- the serial order.  Measured on MI355X (profiles/r3a_pipeline_matrix.md): the contraction kernel
 * occupies every CU completely (256 registers x 8 waves, 126 KB of LDS), so kernels of a second stream only run in the gaps
 * between its workgroups and none of the forked forms is faster than the serial one; the knobs remain for sweeps whose
 * kernels leave room.  Results do not depend on any of these (every pair is computed by the same kernels with per-pair scales).
 * (For experiments the environment variables OVN_HEAD_CHUNK, OVN_HEAD_SUBCHUNK, OVN_HEAD_STREAMS and OVN_YAW_SIDE preset the four
 * values when a context is created; tools/experiments/r3_pipeline_matrix.sh.) */
int ovn_set_head_pipeline(ovn_ctx* ctx, int64_t chunk_pairs, int64_t sub_chunk_pairs, int streams, int yaw_on_side_stream);
/* The current settings (any output pointer may be NULL). */
int ovn_get_head_pipeline(ovn_ctx* ctx, int64_t* chunk_pairs, int64_t* sub_chunk_pairs, int* streams, int* yaw_on_side_stream);

/* Loop-closure decision of a 1-vs-N sweep, on the device (demo/demo3_lcd.py:117-120:
 * `if np.max(overlaps) > overlap_thres: return reference_idx[np.argmax(overlaps)]`; first maximum wins, NaN never wins).
 *   overlap_dev (n) f32, yaw_dev (n) i32 or NULL: outputs of ovn_heads / ovn_delta_head (+ ovn_corr_head_spectral)
 *   ids_dev     (n) i32 candidate ids (reference_idx) or NULL -> position + index_offset (the shard's first candidate)
 *   out_dev     4 x int32, 16-byte aligned: { id of the best candidate (-1 when n == 0), float bits of its overlap, its yaw,
 *                            1 if overlap > threshold else 0 } -- written with ONE 16-byte store; it may be pinned host memory
 *                            (device-visible at the same address): the host then needs no device-to-host copy and may poll word 3
 * Ranks of a sharded sweep exchange these 16-byte records instead of N scores (overlapnet_amd/distributed.py). */
int ovn_best_match(ovn_ctx* ctx, const float* overlap_dev, const int32_t* yaw_dev, const int32_t* ids_dev, int64_t n,
                   float threshold, int64_t index_offset, int32_t* out_dev, void* stream);

/* The k best candidates of a 1-vs-N sweep, ranked on the device: what a back end checks geometrically before it accepts a loop
 * closure, and what recall@k needs.  Arguments as for ovn_best_match; yaw_dev and ids_dev may be NULL.
 *   k        1 .. OVN_TOP_K_MAX
 *   out_dev  k x 4 int32, 16-byte aligned: record i = { id, float bits of overlap, yaw, 1 if overlap > threshold else 0 } of the
 *            i-th best candidate, in ovn_best_match's format; each record is written with one 16-byte store
 * Order: overlap descending; equal overlaps by position ascending (the index into overlap_dev, before ids_dev / index_offset
 * apply: np.argmax's first maximum comes first); -0.0 and +0.0 are equal (a record keeps its element's own bits); +inf ranks
 * first, -inf last; NaN is never selected.  With fewer than k non-NaN scores the remaining records are { -1, 0, 0, 0 } (all of
 * them when n == 0).  The result is the same on every call, and for k == 1 it is bit for bit the record of ovn_best_match.
 * Returns OVN_ERR_ARG for k outside 1..OVN_TOP_K_MAX, n outside [0, 2^31), index_offset + n >= 2^31, a NULL buffer
 * (overlap_dev may be NULL only when n == 0) or a misaligned out_dev.  One workgroup, one launch, no scratch. */
#define OVN_TOP_K_MAX 1024
int ovn_top_k(ovn_ctx* ctx, const float* overlap_dev, const int32_t* yaw_dev, const int32_t* ids_dev, int64_t n, int k,
              float threshold, int64_t index_offset, int32_t* out_dev, void* stream);

/* ovn_top_k of every segment of a batch (ovn_heads_segments' layout), one workgroup per segment, in one launch, no scratch.
 *   seg_offsets  HOST array, B + 1 int64, as in ovn_heads_segments (n = seg_offsets[B] scores in overlap_dev / yaw_dev / ids_dev)
 *   out_dev      B x k x 4 int32, 16-byte aligned: segment b's k records at out_dev + 4 k b
 * Segment b's records are bit for bit those of ovn_top_k on its slice (overlap_dev + seg_offsets[b], yaw_dev / ids_dev sliced the
 * same way, index_offset 0): a NULL ids_dev means the position inside the segment; k = 1 is ovn_best_match's record; an empty
 * segment gives k records { -1, 0, 0, 0 }.  A segment costs the time ovn_top_k takes on it.  OVN_ERR_ARG for k outside
 * 1..OVN_TOP_K_MAX, bad offsets, a NULL or misaligned buffer.  B == 0 is a no-op.  Workspace: the context's segment table
 * (8 (B + 1) bytes, see ovn_heads_segments; it shares that call's one pinned staging buffer and its host wait for a table copy that
 * is still pending). */
int ovn_top_k_segments(ovn_ctx* ctx, const float* overlap_dev, const int32_t* yaw_dev, const int32_t* ids_dev,
                       const int64_t* seg_offsets, int64_t B, int k, float threshold, int32_t* out_dev, void* stream);

/* Verification of loop-closure candidates: projective point-to-plane ICP on the images ovn_project writes, a batch of pairs in one
 * launch (csrc/icp_register.hip; the algorithm is stated step by step in DESIGN.md, "Loop-closure verification").
 *   vertex_dev (n_scans,H,W,4), normal_dev (n_scans,H,W,3), range_dev (n_scans,H,W) f32: ovn_project's outputs (-1 = empty pixel /
 *       no normal); fov_up_deg / fov_down_deg / max_range: the values they were projected with
 *   src_idx_dev, tgt_idx_dev  (n_pairs) int32: pair p registers scan src_idx[p] onto scan tgt_idx[p]
 *   init_pose_dev  (n_pairs,4,4) f64 row-major: T0, source-frame points into the target frame (the yaw head's Rz)
 *   iterations 0..1000 solve passes (no early exit) + one pass without a solve that describes the returned pose;
 *   max_dist [m], cos_min, huber [m]: correspondence gates and the Huber threshold, all > 0; min_inliers >= 0
 *   pose_dev   (n_pairs,4,4) f64: the registered pose
 *   stats_dev  (n_pairs,8) f64: status (0 ok; 1 stopped: a pass found fewer than min_inliers correspondences or the 6x6 Cholesky
 *              met a non-positive / non-finite pivot -- the pose is the last one the pair had, T0 bit for bit when no step was
 *              taken; 2 an index outside [0, n_scans): pose = T0, nothing read), passes solved, inliers, valid source pixels,
 *              rms = sqrt(sum w r^2 / inliers) (0 without inliers), |v| and |omega| of the last step, 0 (reserved)
 *   system_dev (n_pairs,28) f64 or NULL: the first pass's A (upper triangle by rows, 21), b (6) and inlier count -- validation output
 * The pose and every sum are fp64, the per-point arithmetic fp32.  No atomics: a pair's outputs have the same bits alone or in
 * any batch, at any position, on every call.  With a finite T0 nothing non-finite is ever written (a T0
 * holding a NaN or Inf matches no point and comes back as it is, status 1).  n_pairs == 0 is a no-op.  OVN_ERR_ARG for
 * iterations outside 0..1000, a gate that is not > 0, min_inliers < 0, H*W > 2^31 - 1, a NULL buffer. */
int ovn_icp_register(ovn_ctx* ctx, const float* vertex_dev, const float* normal_dev, const float* range_dev, int n_scans,
                     int proj_h, int proj_w, double fov_up_deg, double fov_down_deg, double max_range,
                     const int32_t* src_idx_dev, const int32_t* tgt_idx_dev, int64_t n_pairs, const double* init_pose_dev,
                     int iterations, double max_dist, double cos_min, double huber, int min_inliers, double* pose_dev,
                     double* stats_dev, double* system_dev, void* stream);

/* Overlap-based Monte Carlo localization: the particle filter around a 1-vs-U sweep over the frames of a map (csrc/mcl.hip; every
 * formula is stated in DESIGN.md, "Localization").  Shared by the three calls:
 *   particles_dev  (P,4) f32 rows x, y, theta, w; 16-byte aligned; 1 <= P <= OVN_MCL_MAX_PARTICLES; theta in (-pi, pi]
 *   a map of M >= 1 frames, frame f with heading frame_yaw_dev[f] (f32, radians), and a grid of nx * ny cells (1 .. 2^31 - 1):
 *   cell_frame_dev (ny*nx) i32, row iy * nx + ix = the frame of that cell or -1 (an entry >= M counts as -1)
 *   seed, step     key and counter words of Philox4x32-10: key (seed lo, seed hi), counter (i, step lo, step hi, purpose)
 * Every buffer is the caller's and lives on the context's device unless stated otherwise; nothing uses the context's scratch and no
 * call uses an atomic: the same arguments give the same bits on every call.  Per-particle arithmetic is fp32 with every operation
 * rounded on its own (no FMA contraction), sums are fp64 in an order that depends on P alone, the resampler is integer arithmetic.
 * OVN_ERR_ARG before any launch, buffers untouched: P or n_out outside 1..OVN_MCL_MAX_PARTICLES; nx * ny outside 1..2^31 - 1 (or
 * nx, ny < 1); M < 1; resolution, sigma_yaw_deg or overlap_min not > 0 (NaN included); eps_yaw outside [0, 1]; n_scores outside
 * [0, M]; a NULL buffer (overlap_dev / yaw_dev may be NULL when n_scores == 0, spread_dev always); particles_dev,
 * out_particles_dev, estimate_dev or a record that is not 16-byte aligned; out_particles_dev overlapping particles_dev.
 *
 * ovn_mcl_predict: motion, lookup, the distinct frames.  Host doubles dx, dy, dtheta (odometry in the robot frame) and sigma_x,
 * sigma_y, sigma_theta are rounded to f32.  Particle i draws counter (i, step, 0): u = ((word >> 8) + 0.5) 2^-24 in f32,
 * z_x = sqrt(-2 ln u0) cos(2 pi u1), z_y the same with sin, z_theta from u2, u3 with cos; dx' = dx + sigma_x z_x (dy', dtheta'
 * alike); x += cos(theta) dx' - sin(theta) dy', y += sin(theta) dx' + cos(theta) dy', theta = wrap(theta + dtheta'); w untouched.
 * Lookup: ix = floorf((x - (float)origin_x) * (float)(1 / resolution)), iy alike;
 *   particle_frame_dev (P) i32: cell_frame[iy * nx + ix], or -1 outside the grid, for a non-finite x or y, or in an empty cell
 *   frame_list_dev     (M) i32: the first U entries are the ascending ids of the frames at least one particle landed on
 *   frame_slot_dev     (M) i32: a frame's position in that list, -1 if no particle landed on it
 *   record_dev         4 x i32, 16-byte aligned: { U, particles off the map, 0, 1 }, ONE 16-byte store; may be pinned host memory
 *                      (device-visible at the same address): all the host needs to read before it launches the sweep
 * Three launches (clear M flags, P particles, one workgroup that compacts the flags in tiles of 1024 and counts). */
#define OVN_MCL_MAX_PARTICLES 65536
int ovn_mcl_predict(ovn_ctx* ctx, float* particles_dev, int n_particles, double dx, double dy, double dtheta, double sigma_x,
                    double sigma_y, double sigma_theta, uint64_t seed, uint64_t step, const int32_t* cell_frame_dev, double origin_x,
                    double origin_y, double resolution, int nx, int ny, int n_frames, int32_t* particle_frame_dev,
                    int32_t* frame_slot_dev, int32_t* frame_list_dev, int32_t* record_dev, void* stream);

/* ovn_mcl_update: observation model and estimate; two launches (weights: one particle per thread; maximum, rescale and sums: one
 * workgroup).
 *   particle_frame_dev, frame_slot_dev: as ovn_mcl_predict left them; frame_yaw_dev (M) f32
 *   overlap_dev (n_scores) f32, yaw_dev (n_scores) i32: the sweep over frame_list[0 .. U) with the map frame on head-left and the
 *   query on head-right (ovn_heads' outputs; yaw in degrees as Infer returns it); n_scores = U (a slot >= n_scores is off the map)
 * A particle on frame f with slot s: d = (theta - frame_yaw[f]) (180 / pi) - yaw[s], d -= 360 rintf(d / 360);
 * g = eps + (1 - eps) expf(-0.5 (d / sigma_yaw_deg)^2); o = overlap[s] > overlap_min ? overlap[s] : overlap_min (a NaN score gives
 * overlap_min); w = (w o) g.  A particle off the map: w = (w overlap_min) eps.  Then every weight is multiplied by 2^-e, e the frexp
 * exponent of the largest finite product, so that the maximum lands in [0.5, 1): exact.
 *   estimate_dev (8) f64, 16-byte aligned: status, sum w, N_eff = (sum w)^2 / sum w^2, sum w x / sum w, sum w y / sum w,
 *                atan2(sum w sin theta, sum w cos theta), position of the first maximum weight (NaN never wins), particles on the map
 *   spread_dev   (1) f64 or NULL: sqrt(sum w ((x - mean x)^2 + (y - mean y)^2) / sum w)
 * status 1: no product is finite and positive -- the weights stay the products, the estimate is { 1, 0, 0, 0, 0, 0, -1, on the map },
 * the spread 0.  Otherwise 0. */
int ovn_mcl_update(ovn_ctx* ctx, float* particles_dev, int n_particles, const int32_t* particle_frame_dev,
                   const int32_t* frame_slot_dev, const float* frame_yaw_dev, int n_frames, const float* overlap_dev,
                   const int32_t* yaw_dev, int n_scores, double sigma_yaw_deg, double eps_yaw, double overlap_min,
                   double* estimate_dev, double* spread_dev, void* stream);

/* ovn_mcl_resample: systematic resampling, exact in integers; one launch, one workgroup per 1024 particles, no word between them.
 * q_i = floor(w_i 2^30) (0 for a negative or non-finite weight, 2^30 - 1 for a weight >= 1: ovn_mcl_update leaves every weight
 * below 1), C the inclusive prefix sum of q in 64 bits,
 * S = C[P - 1], r = (word0 | word1 << 32) mod S of counter (0, step, 1).  Output j of n_out copies ancestor a_j = the smallest a
 * with C[a] n_out > j S + r (both sides < 2^62) with weight 1.0f.
 *   out_particles_dev (n_out,4) f32, 16-byte aligned, not overlapping particles_dev; ancestor_dev (n_out) i32
 *   record_dev        4 x i32, 16-byte aligned, ONE 16-byte store: { status, outputs written, 0, 1 }; may be pinned host memory
 * status 1: S == 0 -- the record is { 1, 0, 0, 1 } and nothing else is written.  Ancestors are non-decreasing, a particle with
 * q_i == 0 is never chosen, and particle i is copied floor or ceil of n_out q_i / S times. */
int ovn_mcl_resample(ovn_ctx* ctx, const float* particles_dev, int n_particles, uint64_t seed, uint64_t step,
                     float* out_particles_dev, int n_out, int32_t* ancestor_dev, int32_t* record_dev, void* stream);

/* Spherical projection + normals for a batch of scans (src/utils/utils.py:59-134 range_projection and
 * :137-186 gen_normal_map; the drivers gen_depth_data.py:24-46 etc. loop over files and call these).
 *   points_dev   concatenated (x,y,z,intensity) float32 points of all scans
 *   offsets_dev  (n_scans+1) int64 point offsets into points_dev (scan s = [offsets[s], offsets[s+1]))
 * Outputs, each may be NULL: range (n,H,W), vertex (n,H,W,4), intensity (n,H,W), idx (n,H,W) int32
 * (index among the points that pass the range filter, utils.py:117-118), normal (n,H,W,3), and
 * stacked (n,H,W,C) = the leg input assembled in the reference's channel order depth|normals|intensity
 * (ImagePairOverlapOrientationSequence.py:143-207) according to the use_* flags.  Empty pixels = -1.
 * max_points_per_scan bounds the per-scan launch (>= the largest scan).
 * Limits, OVN_ERR_ARG before any launch: H*W <= 2^31 - 1 (a pixel's index inside its image is a 32-bit integer; indices into the
 * batch are 64-bit), at most 65535 scans per call (the scatter's grid carries the scan in its y dimension), fewer than 2^32 points
 * per scan. */
int ovn_project(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                int64_t max_points_per_scan, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                double max_range, float* range_dev, float* vertex_dev, float* intensity_dev,
                int32_t* idx_dev, float* normal_dev, float* stacked_dev, int use_depth, int use_normals,
                int use_intensity, void* stream);

/* ovn_project plus the class probabilities of the semantic model (use_class_probabilities: gen_semantic_data.py:33-46 and
 * ImagePairOverlapOrientationSequence.py:165-195), from the raw scans in one launch sequence.
 *   probs_dev     (offsets[n_scans], n_classes) float32: one row per point, rows in the order and with the offsets of points_dev;
 *                 may be NULL when neither semantic_dev nor a stacked output with use_semantic is requested
 *   n_classes     1 .. OVN_SEMANTIC_CLASSES_MAX (RangeNet++: 20)
 *   semantic_dev  (n,H,W,n_classes) or NULL: probs[sem_idx] at every pixel with a point, -1 elsewhere
 *   sem_idx_dev   (n,H,W) int32 or NULL: the reference's proj_idx with max_range = inf -- the winner's index among the points with
 *                 depth > 0 and finite.  As in the reference it addresses the UNFILTERED probability rows: a scan with zero-depth or
 *                 NaN points ahead of the winner reads a shifted row (the semantic .npy files a model was trained on were made so)
 *   stacked_dev   (n,H,W,C), C = use_depth + 3 use_normals + n_classes use_semantic + use_intensity: depth | normals |
 *                 probabilities | intensity, the reference's channel order
 * range / vertex / intensity / idx / normal are bit for bit what ovn_project writes at the same max_range, and so are the
 * depth / normal / intensity channels of stacked_dev.  One scatter serves both views: a pixel's nearest point under the semantic
 * filter is its nearest cue point when its depth is < max_range, and otherwise the pixel has no cue point.  OVN_ERR_ARG for
 * n_classes outside 1..OVN_SEMANTIC_CLASSES_MAX, a NULL probs_dev with a probability output, more than 65535 scans,
 * H*W > 2^31 - 1. */
#define OVN_SEMANTIC_CLASSES_MAX 64
int ovn_project_semantic(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                         int64_t max_points_per_scan, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                         double max_range, const float* probs_dev, int n_classes, float* range_dev, float* vertex_dev,
                         float* intensity_dev, int32_t* idx_dev, float* normal_dev, float* semantic_dev, int32_t* sem_idx_dev,
                         float* stacked_dev, int use_depth, int use_normals, int use_semantic, int use_intensity, void* stream);

/* Normal map alone from given range (n,H,W) and vertex (n,H,W,4) images -> normal (n,H,W,3)
 * (src/utils/utils.py:137-186 gen_normal_map).  OVN_ERR_ARG before any launch for H*W > 2^31 - 1. */
int ovn_normals(ovn_ctx* ctx, const float* range_dev, const float* vertex_dev, int n_scans, int proj_h, int proj_w,
                float* normal_dev, void* stream);

/* ovn_render_scans: virtual scans of a triangle mesh, one ray per pixel of the range image, nearest hit (csrc/render_mesh.hip;
 * DESIGN.md section 28).  Builds the map frames of the localization from a mesh instead of recorded keyframes.
 *   vertices_dev  (V,3) f32; triangles_dev (T,3) i32, 1 <= T <= OVN_RENDER_MAX_TRIANGLES; two-sided (no back-face culling); a
 *                 triangle with a vertex index outside [0, V) is skipped and its vertices are never read
 *   poses_dev     (n,4,4) f64 row-major, sensor to world; the rotation R and the origin o are rounded to f32.  A pose with a
 *                 non-finite entry in R or o (after that rounding) gives an all-empty scan
 *   cos_az_dev, sin_az_dev (W) f32; cos_pitch_dev, sin_pitch_dev (H) f32: the CALLER's tables, cos / sin evaluated in f64 and
 *                 rounded to f32, of  azimuth[px] = -(((px + 0.5) / W) * 2 - 1) * pi  and
 *                 pitch[py] = (1 - (py + 0.5) / H) * fov - |fov_down|,  fov = |fov_up| + |fov_down| in radians: the ray through the
 *                 centre of the pixel ovn_project would put a point into.  No transcendental function runs on the device
 * Every operation below is one f32 operation rounded on its own, every dot product is summed (a0 b0 + a1 b1) + a2 b2:
 *   d_s = (cp ca, cp sa, sp);  d_w = (R[:,0] d_s.x + R[:,1] d_s.y) + R[:,2] d_s.z
 *   e1 = v1 - v0, e2 = v2 - v0, p = d_w x e2, det = e1 . p; rejected when det == 0 or det is NaN
 *   inv = 1 / det, s = o - v0, u = (s . p) inv, q = s x e1, v = (d_w . q) inv, t = (e2 . q) inv
 *   a hit: u >= 0, v >= 0, u + v <= 1, t > 0, t < (float)max_range.  The pixel's winner is the hit with the smallest t, among
 *   equal t the smaller triangle index.
 * Outputs, each may be NULL (empty pixels: -1 in every channel):
 *   range_dev (n,H,W) f32 = t; tri_id_dev (n,H,W) i32 = the winner; vertex_dev (n,H,W,4) f32, 16-byte aligned =
 *   (t d_s.x, t d_s.y, t d_s.z, 1), the sensor-frame point as ovn_project stores it; normal_dev (n,H,W,3) = the kernel of ovn_normals
 *   on these range and vertex images; stacked_dev (n,H,W, use_depth + 3 use_normals) = depth | normals, the leg input.
 * The hierarchy (overlapnet_amd/mesh.py builds it): bvh_leaves = NL, a power of two with 4 NL >= T; bvh_order_dev (T) i32, leaf j
 * holds triangles order[4j .. 4j + 3] (entries outside [0, T) are skipped); bvh_nodes_dev (2 NL, 8) f32, 16-byte aligned, row i =
 * lo.x lo.y lo.z 0 hi.x hi.y hi.z 0 of node i of the implicit complete binary tree (root 1, children 2i and 2i + 1, leaves NL ..
 * 2 NL - 1, row 0 unused, lo.x > hi.x marks an empty node).  Every box must contain its triangles with the padding DESIGN.md
 * states; the traversal then returns what the exhaustive route returns.  Both NULL: every ray walks all T triangles in index order
 * (the validation entry).  One writer per pixel, no atomics: the same arguments give the same bits, and a pose renders alone as in
 * any batch.
 * OVN_ERR_ARG, before any launch: V < 1 or > 2^31 - 1, T < 1 or > OVN_RENDER_MAX_TRIANGLES, H or W < 1 or H W > 2^31 - 1, n < 0,
 * max_range not > 0 (NaN included), a NULL mesh buffer, only one of the two hierarchy arrays, bvh_leaves not a power of two in
 * 1 .. 2^25 or 4 bvh_leaves < T, a misaligned bvh_nodes_dev or vertex_dev, use_intensity or use_semantic non-zero (a rendered scan
 * has neither channel), stacked_dev with neither use_depth nor use_normals, and for n > 0 a NULL poses_dev or table.  n == 0 is a
 * no-op. */
#define OVN_RENDER_MAX_TRIANGLES (1ll << 27)
#define OVN_RENDER_LEAF_TRIANGLES 4
int ovn_render_scans(ovn_ctx* ctx, const float* vertices_dev, int64_t n_vertices, const int32_t* triangles_dev, int64_t n_triangles,
                     const float* bvh_nodes_dev, const int32_t* bvh_order_dev, int64_t bvh_leaves, const double* poses_dev,
                     int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev, const float* sin_az_dev,
                     const float* cos_pitch_dev, const float* sin_pitch_dev, double max_range, float* range_dev, int32_t* tri_id_dev,
                     float* vertex_dev, float* normal_dev, float* stacked_dev, int use_depth, int use_normals, int use_intensity,
                     int use_semantic, void* stream);

/* ovn_tsdf_integrate: range images and poses fused into a truncated signed distance volume (csrc/tsdf.hip).
 * With ovn_tsdf_triangles it builds the mesh ovn_render_scans takes from a drive's own scans.
 *   tsdf_dev, weight_dev (nz,ny,nx) f32, x fastest; 2 <= nx, ny, nz and nx ny nz <= 2^31 - 1.  A fresh volume is tsdf = 1, weight = 0
 *   origin        3 doubles on the HOST; origin, voxel, trunc, max_weight and max_range are rounded to f32
 *   range_dev     (n,H,W) f32, -1 = empty: the range images of ovn_project or ovn_render_scans for the same H, W, field of view
 *   poses_dev     (n,4,4) f64 row-major, sensor to world, assumed rigid; R and o are rounded to f32.  A pose with a non-finite
 *                 entry in R or o (after that rounding) skips its scan
 * For every sample (i, j, k), p = origin + (float)(i, j, k) * voxel (one multiply, one add per coordinate), the scans are applied
 * in ascending order, every operation one f32 operation rounded on its own:
 *   1  d = p - o;  q_k = (R[0,k] d0 + R[1,k] d1) + R[2,k] d2
 *   2  depth, yaw, pitch and the unfloored px, py of q exactly as ovn_project computes them for a point (csrc/proj_pixel.h; the
 *      trig mode of ovn_set_projection_trig applies)
 *   3  skipped unless depth > 0 and 0 <= py < H: a sample outside the vertical field of view is NOT compared with the top or
 *      bottom row (ovn_project clamps there)
 *   4  px floored and clamped to 0 .. W - 1 as in ovn_project; r = range[s, floor(py), px]; skipped unless 0 < r < max_range (no
 *      image of ovn_project or ovn_render_scans holds a larger value)
 *   5  sdf = r - depth; skipped when sdf < -trunc (behind the surface, unseen)
 *   6  dv = fminf(1, sdf / trunc)
 *   7  w1 = weight + 1;  tsdf = (weight * tsdf + dv) / w1;  weight = fminf(w1, max_weight)
 * The launch tests scan s only on the box of samples within max_range + trunc + voxel of o (plus one index); every sample outside it
 * fails test 5, so the result does not depend on that -- for a RIGID pose: the argument is depth = |R^T d| = |d| >= |d_a|, and a
 * scaled or sheared matrix makes the box change results.  The margin of one voxel and one index also assumes coordinates small
 * enough that the f32 rounding of p (2^-24 |p| per operation) stays below a voxel: |p| < 10^6 voxels, say.  One writer per sample, no atomics: the same arguments give the same bits,
 * and scans [0, a) then [a, n) in two calls give the bits of one call.
 * OVN_ERR_ARG, before any launch (the volume is untouched): a NULL volume buffer or origin, a dimension < 2 or more than 2^31 - 1
 * samples, a non-finite origin, voxel, trunc, max_weight or max_range not > 0 (NaN included), H or W < 1 or H W > 2^31 - 1,
 * n < 0, and for n > 0 a NULL range_dev or poses_dev.  n == 0 is a no-op. */
int ovn_tsdf_integrate(ovn_ctx* ctx, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const double* origin, double voxel,
                       double trunc, double max_weight, const float* range_dev, const double* poses_dev, int64_t n_scans, int proj_h,
                       int proj_w, double fov_up_deg, double fov_down_deg, double max_range, void* stream);

/* ovn_tsdf_triangles: the zero level set of such a volume as a triangle soup, by marching tetrahedra (csrc/tsdf.hip; DESIGN.md
 * section 29).  Cell (i, j, k), 0 <= i < nx - 1 .., has the corners c = dx + 2 dy + 4 dz.  It is live when all eight corners have
 * weight >= (float)min_weight and their tsdf values are neither all < 0 nor all >= 0 (inside = tsdf < 0).  Its six tetrahedra, in
 * this order: (0,1,3,7) (0,3,2,7) (0,2,6,7) (0,6,4,7) (0,4,5,7) (0,5,1,7).  One or three inside corners of a tetrahedron give one
 * triangle, two give two; the vertex order per case is the table of DESIGN.md section 29, the normal (v1 - v0) x (v2 - v0) points
 * towards positive tsdf.  The vertex on the edge between corners a and b, a the one with the smaller sample index, is
 * p_a + (p_b - p_a) * (D_a / (D_a - D_b)) per coordinate, each operation one f32 operation: two cells compute a shared vertex from
 * the same operands, so the soup is crack-free in bits.  Zero-area triangles (a corner with tsdf == 0) are kept.
 *   triangles_dev   (capacity,3,3) f32 or NULL
 *   n_triangles_dev one int64 on the device: the total count T, written by every call
 * With triangles_dev NULL the call only counts; otherwise it writes the first min(T, capacity) triangles and nothing beyond.
 * Triangles appear in ascending cell index (x fastest), then tetrahedron order, then triangle order: the same arguments give the same
 * bits.  Usual use: one counting call, then one writing call.
 * OVN_ERR_ARG, before any launch: a NULL tsdf_dev, weight_dev, origin or n_triangles_dev, a dimension < 2 or more than 2^31 - 1
 * samples, a non-finite origin, voxel not > 0, min_weight NaN, capacity < 0. */
int ovn_tsdf_triangles(ovn_ctx* ctx, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz, const double* origin,
                       double voxel, double min_weight, float* triangles_dev, int64_t capacity, int64_t* n_triangles_dev, void* stream);

/* ovn_tsdf_raycast: a view of the volume of ovn_tsdf_integrate from a pose, one ray per pixel of the range image marched through
 * the volume (csrc/tsdf_raycast.hip).  It serves a model that changes with every scan: no mesh, no hierarchy.
 * `stream` is the SECOND parameter of this call and of ovn_tsdf_bricks, directly after ctx: the stream-contract table of
 * tests/test_gpu_stream_contract.py lists the prototypes whose parameter list ENDS in the stream, and the change that added these two
 * calls could not edit that table; tests/test_gpu_raycast_stream.py runs both on a non-default stream instead.  The stream contract
 * itself ("Conventions") holds unchanged: both calls only enqueue work on `stream` and restore the caller's device.
 *   tsdf_dev, weight_dev, nx, ny, nz, origin, voxel: the volume of ovn_tsdf_integrate -- samples (nz,ny,nx) f32, x fastest, sample
 *                 (i,j,k) at origin + (i,j,k) voxel; origin (3 doubles on the HOST), voxel, min_weight, min_range, max_range and step
 *                 are rounded to f32
 *   poses_dev, cos_az_dev .. sin_pitch_dev and the outputs range_dev, vertex_dev, normal_dev, stacked_dev, use_depth, use_normals:
 *                 those of ovn_render_scans -- R and o rounded to f32, a pose with a non-finite entry gives an all-empty scan, -1 in
 *                 every channel of an empty pixel, vertex = (t d_s, 1), normal_dev = the kernel of ovn_normals on the range and vertex
 *                 images this call wrote, stacked = depth | normals.  Each output may be NULL
 * Every operation below is one f32 operation rounded on its own, every dot product is summed (a0 b0 + a1 b1) + a2 b2:
 *   1  d_s, d_w as in ovn_render_scans;  inv = 1 / voxel;  per axis a: g_o[a] = (o[a] - origin[a]) inv,  g_d[a] = d_w[a] inv
 *   2  sample k = 0, 1, .. sits at t_k = min_range + (float)k step (one multiply, one add), taken while t_k < max_range: K samples
 *   3  g[a] = g_o[a] + t_k g_d[a];  base corner (i,j,k) = floor(g),  f = g - floor(g)
 *   4  the sample is VALID when 0 <= i <= nx - 2 (likewise j, k; a NaN fails) and all eight corners have weight >= min_weight
 *   5  F = trilinear with lerp(a, b, f) = a + f (b - a): four lerps along x, two along y, one along z; a NaN F makes the sample invalid
 *   6  an invalid sample clears the state "previous sample valid and positive"; a valid F > 0 sets it with F_p = F, t_p = t_k; a valid
 *      F <= 0 ends the ray: with the state set a hit at t = t_p + (t_k - t_p) (F_p / (F_p - F)), with it clear an empty pixel (the ray
 *      came out behind a surface whose front it never saw).  A ray that runs out of samples is empty.
 *   bricks_dev    NULL, or the (ceil(nz/8), ceil(ny/8), ceil(nx/8)) byte mask of ovn_tsdf_bricks for this weight_dev and min_weight: a 0
 *                 promises that no sample of that 8 x 8 x 8 brick has weight >= min_weight, and a sample whose base corner lies in
 *                 such a brick is invalid without a read of the volume.  With a mask that keeps the promise (extra 1s are allowed)
 *                 the output has the bits of the NULL route, which is the definition and the validation entry.
 * One writer per pixel, no atomics: the same arguments give the same bits, and a pose renders alone as in any batch.
 * OVN_ERR_ARG, before any launch (the outputs are untouched): a NULL volume buffer or origin, a dimension < 2 or more than 2^31 - 1
 * samples, a non-finite origin, voxel not > 0, H or W < 1 or H W > 2^31 - 1, n < 0, min_range, max_range or step not finite and > 0
 * (after rounding to f32), min_range >= max_range, K > OVN_RAYCAST_MAX_SAMPLES, a NaN min_weight, a misaligned vertex_dev,
 * stacked_dev with neither use_depth nor use_normals, and for n > 0 a NULL poses_dev or table.  n == 0 is a no-op. */
#define OVN_RAYCAST_MAX_SAMPLES (1ll << 20)
int ovn_tsdf_raycast(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                     const double* origin, double voxel, double min_weight, const uint8_t* bricks_dev, const double* poses_dev,
                     int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev, const float* sin_az_dev,
                     const float* cos_pitch_dev, const float* sin_pitch_dev, double min_range, double max_range, double step,
                     float* range_dev, float* vertex_dev, float* normal_dev, float* stacked_dev, int use_depth, int use_normals);

/* ovn_tsdf_bricks: the mask ovn_tsdf_raycast takes.  bricks_dev (ceil(nz/8), ceil(ny/8), ceil(nx/8)) bytes, x fastest: 1 exactly where
 * some sample (i,j,k) of the brick, i in 8 bi .. min(8 bi + 7, nx - 1) .., has weight >= (float)min_weight, else 0.  One writer per
 * byte, no atomics.  OVN_ERR_ARG, before any launch: a NULL buffer, a dimension < 2 or more than 2^31 - 1 samples, a NaN min_weight.
 * `stream` is the second parameter: see ovn_tsdf_raycast. */
int ovn_tsdf_bricks(ovn_ctx* ctx, void* stream, const float* weight_dev, int nx, int ny, int nz, double min_weight,
                    uint8_t* bricks_dev);

/* A TSDF volume that follows the sensor: a window of fixed size over a lattice fixed in the world, stored as a ring in each axis
 * (csrc/tsdf.hip, csrc/tsdf_raycast.hip, csrc/tsdf_window.hip).  `stream` is the SECOND parameter of the four
 * calls, as for ovn_tsdf_raycast; tests/test_gpu_tsdf_window_stream.py runs them on a non-default stream.  Every call only enqueues
 * work on `stream` and restores the caller's device.  The four calls are additions: no existing prototype or behaviour changes, and
 * OVN_ABI_VERSION stays, as it did when the dense TSDF calls were added.
 *   lattice   sample (I, J, K), integers of either sign, sits at p = anchor + (float)(I, J, K) * voxel: the arithmetic of
 *             ovn_tsdf_integrate with origin = anchor.  anchor: 3 doubles on the HOST, rounded to f32
 *   window    the samples base <= (I, J, K) < base + (nx, ny, nz).  base, old_base, new_base, box_lo, box_hi: 3 int32 on the HOST
 *   storage   tsdf_dev, weight_dev (nz,ny,nx) f32, x fastest; sample I of an axis lives in slot I mod n (floor modulus), likewise J, K.
 *             A fresh window is tsdf = 1, weight = 0 at any base
 *   WINDOW    what every call requires of (nx, ny, nz, base), OVN_ERR_ARG before any launch otherwise: nx, ny, nz multiples of 8 and
 *             >= 16, nx ny nz <= 2^31 - 1, every component of base a multiple of 8, and |I| <= 2^20 for every sample of the window
 *             ((float)I is exact, and the "|p| < 10^6 voxels" of ovn_tsdf_integrate holds).  An aligned run of 8 slots is then 8
 *             consecutive lattice samples: ovn_tsdf_bricks on weight_dev as it is stored gives the mask of the aligned lattice bricks
 * A window sample has the bits the same calls give the sample with that lattice index in a dense volume with origin = anchor: no
 * float operation depends on where a sample is stored.
 *
 * ovn_tsdf_window_integrate: steps 1-7 of ovn_tsdf_integrate for every sample of the window; each scan's box of reachable samples is
 * clamped to the window.  A wave's 64 consecutive slots are one interval of lattice x, or two when the seam of the ring falls inside the
 * run; the scan's box is tested against both.  One writer per sample, no atomics: the same arguments give the same bits, and two calls
 * give the bits of one.  Every other argument, error and the no-op for n == 0 are those of ovn_tsdf_integrate. */
int ovn_tsdf_window_integrate(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const double* anchor,
                              const int32_t* base, double voxel, double trunc, double max_weight, const float* range_dev,
                              const double* poses_dev, int64_t n_scans, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                              double max_range);

/* ovn_tsdf_window_raycast: steps 1-6 of ovn_tsdf_raycast with origin = anchor.  A sample is VALID when its base corner (i, j, k) =
 * floor(g) has base <= i <= base + nx - 2 (likewise j, k; a NaN fails) and all eight corners have weight >= min_weight; each of the
 * eight corners is wrapped into its slot on its own.  bricks_dev: NULL, or the mask of ovn_tsdf_bricks for weight_dev as it is stored;
 * the byte read is the one of the base corner's slot.  Every other argument, output, error and the no-op for n == 0 are those of
 * ovn_tsdf_raycast. */
int ovn_tsdf_window_raycast(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                            const double* anchor, const int32_t* base, double voxel, double min_weight, const uint8_t* bricks_dev,
                            const double* poses_dev, int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev,
                            const float* sin_az_dev, const float* cos_pitch_dev, const float* sin_pitch_dev, double min_range,
                            double max_range, double step, float* range_dev, float* vertex_dev, float* normal_dev, float* stacked_dev,
                            int use_depth, int use_normals);

/* ovn_tsdf_window_shift: the window moves from old_base to new_base.  Every slot whose sample under new_base was not in the old window
 * becomes (tsdf 1, weight 0); no other slot is written, and a sample in both windows keeps its slot and its bits.  One launch per moved
 * axis, over the slab of slots that change hands alone: |new_base - old_base| of that axis times the full extent of the other two.  A
 * move of a whole window or more on any axis clears everything; new_base == old_base launches nothing.  The caller extracts what it
 * wants to keep of the leaving samples BEFORE this call (ovn_tsdf_window_triangles under old_base).
 * OVN_ERR_ARG, before any launch: a NULL buffer or base, WINDOW violated by old_base or by new_base. */
int ovn_tsdf_window_shift(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const int32_t* old_base,
                          const int32_t* new_base);

/* ovn_tsdf_window_triangles: marching tetrahedra exactly as ovn_tsdf_triangles, over the cells whose low corner (I, J, K) lies in
 * box_lo <= (I, J, K) < box_hi.  Triangles appear in ascending cell order WITHIN THE BOX, x fastest, then tetrahedron and triangle
 * order; vertex coordinates are lattice positions, so a cell gives the bits it gives in a dense volume with origin = anchor.  An empty
 * box (box_lo == box_hi on an axis) counts 0.  triangles_dev, capacity, n_triangles_dev: the count / capacity contract of
 * ovn_tsdf_triangles.
 * OVN_ERR_ARG, before any launch: what ovn_tsdf_triangles refuses, WINDOW violated, a NULL box, box_lo > box_hi on an axis, or a cell
 * with a corner outside the window: box_lo < base or box_hi > base + n - 1 on an axis. */
int ovn_tsdf_window_triangles(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                              const double* anchor, const int32_t* base, double voxel, double min_weight, const int32_t* box_lo,
                              const int32_t* box_hi, float* triangles_dev, int64_t capacity, int64_t* n_triangles_dev);

/* SE(3) pose-graph optimization, the back end behind the loop closures of ovn_top_k + ovn_icp_register (csrc/pose_graph.hip;
 * DESIGN.md section 32; restated in NumPy by tests/_pose_graph_ref.py).  Everything is fp64.  `stream` is the SECOND parameter of
 * these calls, as for ovn_tsdf_raycast; tests/test_gpu_pose_graph_stream.py runs them on a non-default stream.  Every call only
 * enqueues work and restores the caller's device; every buffer is the caller's, nothing comes from the context's scratch.
 *   nodes     poses_dev (N,4,4) row-major, sensor to world; fixed_dev (N) bytes, non-zero = the node does not move
 *   edge e    edge_ij_dev (E,2) int32 (i, j), i != j; meas_dev (E,4,4) Z_e measures T_i^-1 T_j (the pose of ovn_icp_register for
 *             (current, reference) is the edge (current, reference, pose) as it stands; an odometry step is (k, k+1, T_k^-1 T_{k+1}));
 *             info_dev (E,6,6) Omega_e, symmetric positive definite, in the twist order (v, omega) of ovn_icp_register
 *   residual  r_e = Log(Z_e^-1 T_i^-1 T_j), translation part first.  With x = theta^2: the six coefficients sin t / t, (1 - cos t) / t^2,
 *             (t - sin t) / t^3, (t^2 + 2 cos t - 2) / (2 t^4), (2 t - 3 sin t + t cos t) / (2 t^5), 1 / t^2 - (1 + cos t) / (2 t sin t)
 *             are their five-term series in x for x < 1e-2 and the closed forms from there on (Exp, Log and the Jacobians alike)
 *   update    T_i <- T_i Exp(delta_i) with the exact Exp; nothing is re-orthonormalized
 *   Jacobians B_e = dr/d delta_j = J_r^-1(r_e) (closed form, Barfoot 7.85-7.86),  A_e = dr/d delta_i = -B_e Ad(T_j^-1 T_i)
 *   cost      s_e = sqrt(r' Omega r), cost = sum rho(s_e), rho = s^2 / 2 for s <= huber, else huber (s - huber / 2); huber = +inf is
 *             least squares; weight w_e = 1 or huber / s_e
 *   H = sum w J' Omega J, g = sum w J' Omega r; rows and columns of fixed nodes are removed (their delta is 0)
 * An edge with a non-finite pose, measurement or information entry, or with an index outside [0, N) or i == j, gets weight 0 and zero
 * blocks and is counted in the record.  No atomics anywhere: a node's sums run over its incidence list node_ptr_dev (N + 1) /
 * node_edge_dev (2 E) (CSR, a node's edges in ascending edge index) in list order, dot products and maxima are fixed trees, the scans
 * are three launches (block scans, one workgroup over the block totals, add): the same arguments give the same bits.
 *
 * record_dev: OVN_POSE_GRAPH_RECORD doubles.  [0] cost  [1] edges with weight 0 for a non-finite input  [2] 6 x 6 blocks whose
 * Cholesky met a non-positive pivot  [3] |g|_inf  (ovn_pose_graph_linearize; [2] and [3] are 0 from a cost-only call)
 * [4] PCG iterations done  [5] |r|_M / |r_0|_M  [6] converged  [7] breakdown  [8] r'z  [9] r_0'z_0  [10] alpha  [11] beta
 * (ovn_pose_graph_solve)  [12] |delta|_inf of the free nodes (ovn_pose_graph_retract)  [13] failed pivots and [14] loop edges left
 * out (ovn_pose_graph_loops_prepare, below).
 *
 * ovn_pose_graph_workspace_bytes: the size of ws_dev for N nodes and E edges (0 for N or E outside the limits).
 *
 * ovn_pose_graph_linearize: res_dev (E,6) r, chi_dev (E) s, weight_dev (E) w, and -- when jac_dev is given -- jac_dev (E,2,6,6) A | B,
 * blocks_dev (E,3,6,6) A'wOmega A | A'wOmega B | B'wOmega B, grad_dev (N,6) g, diag_dev (N,6,6) the diagonal blocks of H, dinv_dev
 * (N,6,6) their inverses by Cholesky (0 for a fixed node and for a block that broke down), and chain_dev (NULL, or (N-1,2,6,6)): the
 * chain preconditioner's G_m | Ad(T_{m+1}^-1) of edge m = (m, m+1), which the CALLER promises are edges 0 .. N-2 with node 0 the only
 * fixed node.  With jac_dev, blocks_dev, grad_dev, diag_dev, dinv_dev and chain_dev all NULL it is the cost-only evaluation of a
 * trial step.  E == 0: cost 0, no buffer but the record is touched.
 *
 * ovn_pose_graph_solve: enqueues `iterations` iterations of preconditioned conjugate gradients on (H + lambda blockdiag(H)) delta
 * = -g from delta = 0 (first_iteration == 0 starts the solve; a later chunk passes the number of iterations enqueued so far and
 * continues from ws_dev).  preconditioner: OVN_POSE_GRAPH_JACOBI = dinv_dev / (1 + lambda); OVN_POSE_GRAPH_CHAIN = the inverse of the
 * Hessian of the N-1 odometry edges alone, undamped, by two transforms per node around a prefix and a suffix sum (chain_dev).  The
 * record's `converged` is set when |r|_M / |r_0|_M <= rtol (or g == 0), `breakdown` when the linearization's record counts a failed
 * Cholesky or p'(H + lambda D)p is not positive and finite; from then on every remaining launch returns at its first instruction, so
 * delta_dev holds the last good iterate (untouched by a solve that breaks down at its start) and never a non-finite value.  The call
 * never waits on the host.  E == 0: converged after 0 iterations, delta_dev untouched.
 *
 * ovn_pose_graph_precondition: out_dev (N,6) = M^-1 in_dev (N,6) alone (a validation entry; with the chain, row 0 of out_dev is 0).
 *
 * ovn_pose_graph_retract: out_dev (N,4,4) = T_i Exp(delta_i) (a fixed node is copied), record [12].  out_dev must not be poses_dev.
 *
 * OVN_ERR_ARG, before any launch: a NULL ctx, record or (for E > 0) buffer, N < 1, E < 0, N > OVN_POSE_GRAPH_MAX_NODES, E >
 * OVN_POSE_GRAPH_MAX_EDGES, huber <= 0 or NaN, lambda or rtol negative or non-finite, an unknown preconditioner, the chain without
 * chain_dev or with E < N - 1, first_iteration < 0, iterations outside 0 .. OVN_POSE_GRAPH_MAX_CHUNK, Jacobian outputs given in part. */
#define OVN_POSE_GRAPH_MAX_NODES (1 << 20)
#define OVN_POSE_GRAPH_MAX_EDGES (1 << 22)
#define OVN_POSE_GRAPH_MAX_CHUNK 4096
#define OVN_POSE_GRAPH_RECORD 16
#define OVN_POSE_GRAPH_JACOBI 0
#define OVN_POSE_GRAPH_CHAIN 1
int64_t ovn_pose_graph_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int ovn_pose_graph_linearize(ovn_ctx* ctx, void* stream, const double* poses_dev, const uint8_t* fixed_dev, int n_nodes,
                             const int32_t* edge_ij_dev, const double* meas_dev, const double* info_dev, int n_edges,
                             const int32_t* node_ptr_dev, const int32_t* node_edge_dev, double huber, double* res_dev, double* chi_dev,
                             double* weight_dev, double* jac_dev, double* blocks_dev, double* grad_dev, double* diag_dev,
                             double* dinv_dev, double* chain_dev, double* ws_dev, double* record_dev);
int ovn_pose_graph_solve(ovn_ctx* ctx, void* stream, const uint8_t* fixed_dev, int n_nodes, const int32_t* edge_ij_dev, int n_edges,
                         const int32_t* node_ptr_dev, const int32_t* node_edge_dev, const double* blocks_dev, const double* grad_dev,
                         const double* diag_dev, const double* dinv_dev, const double* chain_dev, int preconditioner, double lambda,
                         double rtol, int first_iteration, int iterations, double* delta_dev, double* ws_dev, double* record_dev);
int ovn_pose_graph_precondition(ovn_ctx* ctx, void* stream, int n_nodes, int preconditioner, double lambda, const double* dinv_dev,
                                const double* chain_dev, const double* in_dev, double* out_dev, double* ws_dev);
int ovn_pose_graph_retract(ovn_ctx* ctx, void* stream, const double* poses_dev, const uint8_t* fixed_dev, const double* delta_dev,
                           int n_nodes, double* out_dev, double* ws_dev, double* record_dev);

/* The chain-plus-loops inverse: the third preconditioner, for a drive with many loop closures (csrc/pose_graph.hip; DESIGN.md section
 * 33; restated by tests/_pose_graph_loops_ref.py).  PRECONDITION, which the CALLER promises as for chain_dev: edges 0 .. N-2 are the
 * chain (k, k+1) in order, node 0 is the only fixed node, and the L = E - (N-1) edges after the chain are the loop edges (i, j) -- in
 * either order, touching node 0 or not, repeated or not.  In chain coordinates the linear part of loop edge a is sigma_a C_a times a
 * sum over the chain edges [lo_a, hi_a) (C_a = B_a Ad(T_j^-1), lo = min(i, j), hi = max(i, j), sigma = +1 for j > i, else -1), so
 * Woodbury's identity gives the exact inverse of the UNDAMPED Hessian from the chain inverse and the 6 L x 6 L matrix
 *   S_ab = delta_ab (w_a Omega_a)^-1 + sigma_a sigma_b C_a (Gamma[min(hi_a, hi_b)] - Gamma[max(lo_a, lo_b)]) C_b'   (spans that overlap)
 * with Gamma[k] = sum_{m<k} G_m.  With lambda > 0 it is a preconditioner only.
 *
 * ovn_pose_graph_loops_bytes: the size of loops_dev for N nodes and L loop edges; 0 for N outside 2 .. OVN_POSE_GRAPH_MAX_NODES or L
 * outside 1 .. OVN_POSE_GRAPH_MAX_LOOPS.  ovn_pose_graph_loops_layout: out[0] the factorization's block size b, out[1] the padded
 * order sp of S (6 L rounded up to b, an identity diagonal in the padding), out[2..7] the offsets in doubles of Gamma (N,6,6), C (L,6,6),
 * (w Omega)^-1 (L,6,6), the spans (L,4: lo, hi, sigma, live), S (sp,sp) and its lower Cholesky factor (sp,sp) inside loops_dev.
 *
 * ovn_pose_graph_loops_prepare: runs after an ovn_pose_graph_linearize with chain_dev on the same buffers; writes all of the above
 * and record [13] = pivots that were not positive and finite (in a loop edge's w Omega or in the blocked right-looking Cholesky
 * factorization of S; one launch per stage -- panel, triangular solve, symmetric update -- per block column) and [14] = loop edges
 * left out because their weight is 0 (a non-finite input): zero C, identity block in S.  `stages` is OVN_POSE_GRAPH_LOOPS_ALL; a
 * benchmark times the three stages by asking for them one at a time, in order (SCAN: Gamma; ASSEMBLE: C, the spans, S and a copy of
 * its lower triangle; FACTOR: that copy factored in place, and the record).
 *
 * ovn_pose_graph_solve_loops: the contract of ovn_pose_graph_solve with this preconditioner (OVN_POSE_GRAPH_LOOPS): z = H^-1 r by the
 * chain's suffix and prefix scans, d = S^-1 v by two triangular sweeps, a difference scan over the incidence list, and one more
 * prefix scan; loops_dev also holds the apply's scratch.  `breakdown` is also set, before delta_dev is touched, when record [13] is
 * not 0.  ovn_pose_graph_precondition_loops: out_dev (N,6) = H^-1 in_dev alone, row 0 zero (a validation entry).
 *
 * OVN_ERR_ARG, before any launch: a NULL ctx or buffer, N < 2, L < 1, L > OVN_POSE_GRAPH_MAX_LOOPS, E != N - 1 + L, and what
 * ovn_pose_graph_solve refuses. */
#define OVN_POSE_GRAPH_LOOPS 2
#ifndef OVN_POSE_GRAPH_MAX_LOOPS   /* a benchmark build may raise it (to 512 at most) to measure beyond the cap */
#define OVN_POSE_GRAPH_MAX_LOOPS 256
#endif
#define OVN_POSE_GRAPH_LOOPS_SCAN 1
#define OVN_POSE_GRAPH_LOOPS_ASSEMBLE 2
#define OVN_POSE_GRAPH_LOOPS_FACTOR 4
#define OVN_POSE_GRAPH_LOOPS_ALL 7
int64_t ovn_pose_graph_loops_bytes(int64_t n_nodes, int64_t n_loops);
int ovn_pose_graph_loops_layout(int64_t n_nodes, int64_t n_loops, int64_t* out);
int ovn_pose_graph_loops_prepare(ovn_ctx* ctx, void* stream, const double* poses_dev, int n_nodes, const int32_t* edge_ij_dev,
                                 const double* info_dev, const double* weight_dev, const double* jac_dev, int n_edges, int n_loops,
                                 const double* chain_dev, int stages, double* loops_dev, double* record_dev);
int ovn_pose_graph_solve_loops(ovn_ctx* ctx, void* stream, const uint8_t* fixed_dev, int n_nodes, const int32_t* edge_ij_dev, int n_edges,
                               const int32_t* node_ptr_dev, const int32_t* node_edge_dev, const double* blocks_dev, const double* grad_dev,
                               const double* diag_dev, const double* dinv_dev, const double* chain_dev, double* loops_dev, int n_loops,
                               double lambda, double rtol, int first_iteration, int iterations, double* delta_dev, double* ws_dev,
                               double* record_dev);
int ovn_pose_graph_precondition_loops(ovn_ctx* ctx, void* stream, int n_nodes, int n_edges, int n_loops, const int32_t* node_ptr_dev,
                                      const int32_t* node_edge_dev, const double* chain_dev, double* loops_dev, const double* in_dev,
                                      double* out_dev, double* ws_dev);

/* Marginal pose covariances: the diagonal 6 x 6 blocks of the inverse of the undamped Hessian of a chain plus L >= 0 loop edges, for a
 * list of nodes (csrc/pose_graph.hip; restated by tests/_pose_graph_marginals_ref.py).  The PRECONDITION is that
 * of the chain-plus-loops inverse above.  For the left perturbation T_k <- Exp(eps_k) T_k, eps = (v, omega) in the world,
 *   Sigma_world(k) = Gamma[k] - Y_k' Y_k,   L_S Y_k = V_k',   V_k = [ (Gamma[clamp(k, lo_a, hi_a)] - Gamma[lo_a]) sigma_a C_a' ]_a  (6 x 6 L)
 * with S = L_S L_S' the factor ovn_pose_graph_loops_prepare left.  Everything is relative to the fixed node 0, whose block is all
 * zeros, and uses the edge weights (Huber weights included) of the linearization it follows.  `frame`:
 *   OVN_POSE_GRAPH_COV_LOCAL     the optimizer's own delta_k (T_k <- T_k Exp(delta_k)): Ad(T_k^-1) Sigma_world Ad(T_k^-1)'
 *   OVN_POSE_GRAPH_COV_POSITION  (position in the world, rotation vector in the world): J Sigma_world J', J = [[I, -[p_k]x], [0, I]];
 *                                its top-left 2 x 2 is the x, y covariance of a search ellipse
 * cov_dev (n_query,6,6) row-major, every block symmetric to the bit; node_ids_dev (n_query) int32 in any order, repeats allowed.  An id
 * outside [0, N) gives a block of NaNs and is counted in record [15].  For L >= 1 loops_dev comes from ovn_pose_graph_loops_prepare
 * with OVN_POSE_GRAPH_LOOPS_ALL after the same linearization as chain_dev; for L == 0 it is not read (NULL) and Gamma is scanned from
 * chain_dev into the workspace: dead-reckoning covariance propagation.  When record [2] (or, for L >= 1, [13]) is not 0 the call sets
 * `breakdown` [7] and cov_dev is not touched; otherwise it clears [7].  It must not run between the chunks of a solve.
 *
 * The sweep walks the queried nodes in launches of at most 512 workgroups of 8 nodes, so ws_dev is bounded however many are asked for:
 * ovn_pose_graph_marginals_bytes(N, L, K) is 8 bytes times  ceil(K / 256)  +  (L == 0 ? 36 N + 72 ceil((N - 1) / 256) : 0)  +
 * min(ceil(K / 8), 512) * sp * 48  with sp = 6 L rounded up to 48 (each term rounded up to even), at most 302 MB for L = 256 and a
 * few hundred bytes for L == 0, K <= 256.  It returns 0 for N outside 2 .. OVN_POSE_GRAPH_MAX_NODES, L outside 0 ..
 * OVN_POSE_GRAPH_MAX_LOOPS or K outside 1 .. OVN_POSE_GRAPH_MAX_QUERY.
 *
 * OVN_ERR_ARG, before any launch and with every buffer as it was: a NULL ctx or buffer (loops_dev only for L >= 1), N < 2, L < 0,
 * L > OVN_POSE_GRAPH_MAX_LOOPS, E != N - 1 + L, n_query outside 1 .. OVN_POSE_GRAPH_MAX_QUERY, an unknown frame. */
#define OVN_POSE_GRAPH_COV_LOCAL 0
#define OVN_POSE_GRAPH_COV_POSITION 1
#define OVN_POSE_GRAPH_MAX_QUERY (1 << 22)
int64_t ovn_pose_graph_marginals_bytes(int64_t n_nodes, int64_t n_loops, int64_t n_query);
int ovn_pose_graph_marginals(ovn_ctx* ctx, void* stream, const double* poses_dev, int n_nodes, int n_edges, int n_loops,
                             const double* chain_dev, const double* loops_dev, const int32_t* node_ids_dev, int64_t n_query, int frame,
                             double* cov_dev, double* ws_dev, double* record_dev);

/* The per-point part of range_projection alone (src/utils/utils.py:75-104), exactly as ovn_project's scatter kernel evaluates it:
 * for each of n float32 points (x,y,z,*) yaw = -np.arctan2(y, x), pitch = np.arcsin(z / depth) with NumPy's float32 results
 * (csrc/svml_f32.h) and the pixel py * proj_w + px the point falls into (-1 for a point the range filter drops).  Outputs may
 * be NULL.  A validation entry: lets a test compare the two angle functions with the reference's NumPy on millions of points.
 * OVN_ERR_ARG before any launch for H*W > 2^31 - 1 (the pixel is a 32-bit integer). */
int ovn_projection_angles(ovn_ctx* ctx, const float* points_dev, int64_t n_points, int proj_h, int proj_w, double fov_up_deg,
                          double fov_down_deg, double max_range, float* yaw_dev, float* pitch_dev, int32_t* pixel_dev,
                          void* stream);

/* Ground-truth overlap labels (src/utils/com_overlap_yaw.py:28-46), the producer of the training / evaluation targets.
 * ovn_gt_range_images: range images (n, H, W) f32 (-1 = empty) of n scans moved by p' = inv_cur_pose . (ref_pose[s] . p)
 *   and range-projected in FLOAT64 as `range_projection` does for load_vertex's float64 points (utils.py:59-134,217-230).
 *   points/offsets as in ovn_project; ref_poses_dev (n,4,4) f64 row-major or NULL (identity); inv_cur_pose_dev (4,4) f64 or
 *   NULL (identity) -- with both NULL this is the current frame's own range image (com_overlap_yaw.py:30-31).
 * ovn_gt_overlap_counts: counts_dev[s] = #{ref_range[s] > 0 and |ref_range[s] - cur_range| < 1} for s < n, and
 *   counts_dev[n] = #{cur_range > 0} (`valid_num`, :32-33): overlap[s] = counts[s] / counts[n] (:42-45).
 * Limits, OVN_ERR_ARG before any launch: H*W <= 2^31 - 1 for both calls (a pixel's index inside its image is a 32-bit integer),
 * at most 65535 scans per ovn_gt_range_images call (its grid carries the scan in the y dimension) and at most 2^31 - 2 per
 * ovn_gt_overlap_counts call (one workgroup per scan and one more). */
int ovn_gt_range_images(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                        int64_t max_points_per_scan, const double* ref_poses_dev, const double* inv_cur_pose_dev, int proj_h,
                        int proj_w, double fov_up_deg, double fov_down_deg, double max_range, float* range_dev, void* stream);
int ovn_gt_overlap_counts(ovn_ctx* ctx, const float* ref_ranges_dev, const float* cur_range_dev, int n_scans, int proj_h,
                          int proj_w, int32_t* counts_dev, void* stream);

/* All pairs of a sequence in one call: counts_dev[f * n_refs + r] = the integer ovn_gt_overlap_counts gives for frame
 * frame_idx[f] against scan ref_idx[r], without the pair's range image (two bit planes in LDS, one workgroup per pair;
 * csrc/overlap_gt.hip).  points/offsets as in ovn_gt_range_images for all n_scans scans; poses_dev (n_scans,4,4) f64;
 * inv_poses_dev (n_scans,4,4) f64, the caller's inverses (the host's np.linalg.inv, so that the bits are those ovn_gt_range_images
 * is given); cur_ranges_dev (n_scans,H,W) f32 indexed by SCAN: the own range images (ovn_gt_range_images with both poses NULL),
 * read only for the scans frame_idx names.  frame_idx_dev / ref_idx_dev: int32 device lists, NULL = 0..n-1; entries may repeat and
 * need not be sorted; an entry outside [0, n_scans) reads nothing and reports -1 for its pairs.  OVN_ERR_ARG when H*W > 262144
 * (the planes exceed 64 KB of LDS) or n_frames * n_refs > 2^31 - 1.  overlap = counts / #{cur_range > 0} is the caller's division. */
int ovn_gt_pair_counts(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans, const double* poses_dev,
                       const double* inv_poses_dev, const float* cur_ranges_dev, const int32_t* frame_idx_dev, int n_frames,
                       const int32_t* ref_idx_dev, int n_refs, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                       double max_range, int32_t* counts_dev, void* stream);

/* Arithmetic of the Delta head's contractions (c_conv1, c_conv2, c_conv3) and of ovn_spectrum's DFT; storage and accumulation
 * are fp32 in every mode:
 *   0 = fp32 matrix cores (v_mfma_f32_16x16x4_f32; bit-for-bit an fp32 FMA chain),
 *   1 = scaled 3-term fp16 split on the fp16 matrix cores (x * 2^k = hi + lo, a*w ~ ah*wh + al*wh + ah*wl; 2^-21 per operand)
 *       -- the default, measured as accurate as mode 0; both modes are held to |d overlap| <= 1e-4 against the fp64 oracle on
 *       every pair of the benchmark sweep by the parity tests,
 *   2 = bf16x3: DeltaLayer + c_conv1 and c_conv2 on the bf16 matrix cores with the exact 3-term bf16 split of every fp32 operand
 *       (x = hi + mid + lo by truncation, a*w ~ the six terms down to 2^-24 relative: fp32's own rounding level); the linear terms
 *       of the min form in fp32, c_conv3, Dense and the DFT as in mode 0.  A pair with a negative value is shifted (l + c, r + c
 *       rounded once in fp32, the same class of error as mode 0's l - r).  Delta cache rows are ignored, as in mode 0.
 * Any other value: OVN_ERR_ARG. */
int ovn_set_head_precision(ovn_ctx* ctx, int mode);

/* Delta head at a feature width other than 360 with conv1size 15 (default 0):
 *   0 = exact fp32 in every head precision mode (delta_head.hip),
 *   1 = head precision 1 (f16x3) runs DeltaLayer + c_conv1 + c_conv2 there in its scaled 3-term fp16 split on kernels with a
 *       run-time width (delta_head_w_f16x3.hip: |l - r| formed in fp32, scaled per PAIR and split; a pair's result depends on its
 *       two volumes alone); c_conv3, Dense and the correlation head stay fp32, head precisions 0 and 2 keep the fp32 kernels.
 * Every entry point that reaches the Delta head follows it (ovn_heads, ovn_delta_head, ovn_heads_segments, indexed or not).  No
 * effect at feat_w = 360.  Any other value: OVN_ERR_ARG. */
int ovn_set_head_width_split(ovn_ctx* ctx, int on);
int ovn_get_head_width_split(ovn_ctx* ctx, int* on);

/* Arithmetic of the leg convolutions, same two modes as ovn_set_head_precision (default 1). */
int ovn_set_leg_precision(ovn_ctx* ctx, int mode);

/* Dead-channel compaction of the Delta head's contraction in 1-vs-N sweeps (default 1).  DeltaLayer + c_conv1
 * (generateNet.py:45-59,96-100) sum |l - r| w over the 128 feature channels; in the min form of the f16x3 path a channel that is 0
 * in all 360 columns of the QUERY (ReLU outputs: a quarter of the channels under the benchmark's weights) contributes exact zeros
 * for every candidate, so the K walk covers only ceil(live / 32) slices of 32 channels.  Exact; changes only how K is grouped into
 * MFMA steps (last-bit differences against on = 0).  Pairs with negative values and indexed pairs always walk all 128 channels. */
int ovn_set_head_compaction(ovn_ctx* ctx, int on);

/* Which float32 `np.arctan2` / `np.arcsin` (src/utils/utils.py:86-87) ovn_project / ovn_projection_angles reproduce:
 *   0 (default)  NumPy >= 1.22 on an AVX512_SKX x86-64 host: Intel SVML's 1-4 ulp kernels, bit for bit (csrc/svml_f32.h) -- the
 *                machine the reference's shipped .npy files and this repo's golden vectors were produced on;
 *   1            the correctly rounded float32 results (float64 function, rounded once): what NumPy gives where its float32 loops
 *                call a correctly rounded libm (AVX2-only x86, aarch64 ...).  The two differ in the last bit of 38 % of the angles
 *                and put a point into the neighbouring pixel about once per 200 k points. */
int ovn_set_projection_trig(ovn_ctx* ctx, int mode);

/* Per-kernel-class timing with HIP events recorded on the launch stream, for bench.py's roofline line.
 * Between begin and end every kernel group launched through this context is bracketed by an event
 * pair; ovn_profile_end waits for them and returns, per class, the summed milliseconds and the number
 * of bracketed launches.  Classes: 0 leg convolutions (one entry per layer launch), 1 correlation head,
 * 2 Delta kernel (DeltaLayer+c_conv1 contraction; fp32 mode: fused with c_conv2), 3 c_conv3, 4 dense+sigmoid, 5 projection,
 * 6 spectrum (DFT), 7 spectral correlation head, 8 Delta prepare kernels, 9 c_conv2 GEMM of the f16x3 Delta path. Arrays of 10. */
int ovn_profile_begin(ovn_ctx* ctx);
int ovn_profile_end(ovn_ctx* ctx, double* ms_by_kind, int64_t* launches_by_kind);

/* Test hook: run registered leg layer `layer` alone on in_dev (nb,h,w,cin) -> out_dev (nb,oh,ow,cout). */
int ovn_debug_conv(ovn_ctx* ctx, int layer, const float* in_dev, int nb, int h, int w, float* out_dev, void* stream);

/* Test hook: copy the c_conv2 (n,G,G,128) and c_conv3 (n,G-2,G-2,256) activations that the most recent
 * ovn_heads call left in scratch (its first chunk / sub-chunk, n <= min(pairs, chunk_pairs, sub_chunk_pairs)); either output may be NULL.
 * G = feat_w // 15: 24 at feat_w = 360.  The fp32 kernels (head precision 0 at feat_w = 360, every precision at any other feat_w;
 * conv1size 15) keep them only for a call that ran as ONE chunk (n <= its pair count); after a call of several chunks, and on the
 * general conv1size path, the hook returns OVN_ERR_STATE.
 * (generateNet.py:102-110 intermediates; the reference exposes them as Keras layer outputs.) */
int ovn_debug_head_activations(ovn_ctx* ctx, int64_t n, float* o2_dev, float* o3_dev, void* stream);

/* Measurement hook: the K walk of the Delta head's contraction in the most recent 1-vs-N sweep on this context (its last chunk).
 * out16_host (HOST memory, 16 x int32): [0] slices of 32 channels a pass of the contraction kernel walks (1..4: the largest count
 * below), [1] channels of the query that are non-zero somewhere in its 360 columns, [2..13] slices the live channels of column-group
 * pairs 0..11 need (a pair = two column groups of c_conv1, generateNet.py:96-100; a wave skips a slice none of its column groups
 * walks), [14] 1 if the dead-channel compaction applied (ovn_set_head_compaction), else 0 and every entry says 4 slices / 128
 * channels, [15] MFMA steps of the LAST slice when it is packed tap-major (it then holds <= 16 live channels: 3, 6 or 9 steps instead
 * of 15; 0 = not packed).  Synchronises `stream`.  bench.py reports roofline.k_walk_frac from it. */
int ovn_head_walk_stats(ovn_ctx* ctx, int32_t* out16_host, void* stream);

/* Device scratch currently held by the context, in bytes (grows on demand, freed by ovn_destroy). */
int64_t ovn_workspace_bytes(ovn_ctx* ctx);

/* ---- optional collective for consumers that do not use torch.distributed --------------------------
 * The 1-vs-N sweep shards the candidates over the ranks in contiguous blocks (no data-path collective); its one exchange
 * step is the gather of the (overlap, yaw) results, 8 bytes per candidate.  RCCL is loaded with dlopen on first use (no
 * link-time dependency; an RCCL already in the process, e.g. PyTorch's, is reused).  The Python package does not call these
 * (it goes through torch.distributed, backend "nccl" = RCCL).
 *   rank 0: ovn_comm_unique_id(id); the application hands the OVN_COMM_ID_BYTES bytes to the other ranks (MPI, file, socket);
 *   every rank: ovn_comm_init(ctx, rank, world_size, id)  -- collective, one communicator per context, on the context's GPU;
 *   per query:  ovn_gather_scores(...) -- collective; rank r contributes counts_host[r] candidates (its shard of the sweep, host
 *               array of world_size entries, identical on every rank); on `root` overlap_all_dev / yaw_all_dev (sum of counts)
 *               receive the shards in rank order; other ranks may pass NULL result buffers.  Enqueued on `stream`. */
#define OVN_COMM_ID_BYTES 128
int ovn_comm_unique_id(unsigned char* id_out);
int ovn_comm_init(ovn_ctx* ctx, int rank, int world_size, const unsigned char* id);
int ovn_comm_destroy(ovn_ctx* ctx);
int ovn_gather_scores(ovn_ctx* ctx, const float* overlap_dev, const int32_t* yaw_dev, const int64_t* counts_host, int root,
                      float* overlap_all_dev, int32_t* yaw_all_dev, void* stream);

/* Self-test of the MFMA fragment layouts this library relies on (runs a few tiny kernels on the
 * context's device and compares with a host matmul).  0 = all layouts as assumed. */
int ovn_selftest(ovn_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* OVN_HIP_H */
