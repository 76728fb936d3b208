// extern "C" surface of libovn_hip.so (declared in include/ovn_hip.h) -- argument checking, weight
// re-tiling, scratch management and the launch sequences.  No torch types anywhere: plain pointers.
#include <stdarg.h>
#include <mutex>
#include <set>
#include <utility>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include "ovn_internal.h"

int ovn_allow_dynamic_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  OVN_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({kernel, dev})) return OVN_OK;
  OVN_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done.insert({kernel, dev});
  return OVN_OK;
}

static thread_local char g_err[1024] = "";

void ovn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

void scratch_overwritten(ovn_ctx* ctx) {
  ctx->dbg_o2 = ctx->dbg_o3 = nullptr;
  ctx->dbg_partial = nullptr;
  ctx->dbg_o2max = nullptr;
  ctx->dbg_n = 0;
  ctx->dbg_live = nullptr;
}

// One scratch block per context, grown on demand and never shrunk.  Growing it synchronises `stream` and frees the old block
// (hipFree waits for the device), so a context must be driven from ONE stream at a time (include/ovn_hip.h says so).
int ovn_ws_reserve(ovn_ctx* ctx, size_t bytes, hipStream_t stream) {
  if (bytes <= ctx->ws_bytes) return OVN_OK;
  if (ctx->ws) {
    OVN_HIP_CHECK(hipStreamSynchronize(stream));  // earlier launches may still use the old block
    OVN_HIP_CHECK(hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    scratch_overwritten(ctx);
  }
  const size_t want = bytes + bytes / 8;  // a little headroom so near-equal requests do not thrash
  OVN_HIP_CHECK(hipMalloc(&ctx->ws, want));
  ctx->ws_bytes = want;
  return OVN_OK;
}

// Width of the context's feature volumes: the leg's output once finalized, the reference's 360 before (a context that registers head
// weights without a leg keeps the behaviour it always had)
static int ctx_feat_w(const ovn_ctx* ctx) { return ctx->finalized ? ctx->feat_w : OVN_FEAT_W; }

// Scratch of the leg calls: `nbuf` (1 or 2) activation buffers of buf_elems floats | fp64 running sums | the partials of
// ovn_leg_layer_backward (ovn_leg_grad_part_bytes)
struct LegScratch {
  float* buf[2] = {nullptr, nullptr};
  double *acc = nullptr, *part = nullptr;
  LegScratch() = default;
  LegScratch(OvnCarver& c, size_t buf_elems, int nbuf, size_t acc_elems, size_t part_bytes) {
    for (int i = 0; i < nbuf; ++i) buf[i] = c.take<float>(buf_elems);
    acc = c.take<double>(acc_elems);
    part = reinterpret_cast<double*>(c.take<char>(part_bytes));
  }
};

extern "C" {

int ovn_abi_version(void) { return OVN_ABI_VERSION; }

const char* ovn_last_error(void) { return g_err; }

int ovn_create(int device_id, int in_h, int in_w, int in_c, ovn_ctx** out) {
  OVN_REQUIRE(out != nullptr, OVN_ERR_ARG, "ovn_create: out is NULL");
  OVN_REQUIRE(in_h > 0 && in_w > 0 && in_c > 0, OVN_ERR_ARG, "ovn_create: bad input shape %dx%dx%d", in_h, in_w, in_c);
  int ndev = 0;
  OVN_HIP_CHECK(hipGetDeviceCount(&ndev));
  OVN_REQUIRE(device_id >= 0 && device_id < ndev, OVN_ERR_ARG, "ovn_create: device %d not present (%d devices)", device_id, ndev);
  OVN_ON_DEVICE(device_id);
  hipDeviceProp_t prop;
  OVN_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
  OVN_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, OVN_ERR_STATE,
              "ovn_create: this library is built for gfx950 only, device %d is %s", device_id, prop.gcnArchName);
  ovn_ctx* c = new ovn_ctx();
  c->device = device_id;
  c->in_h = in_h;
  c->in_w = in_w;
  c->in_c = in_c;
  // experiment knobs (tools/experiments): the defaults are the measured best, ovn_set_head_pipeline is the API
  if (const char* e = getenv("OVN_HEAD_CHUNK")) c->head_chunk = atoll(e) > 0 ? atoll(e) : c->head_chunk;
  if (const char* e = getenv("OVN_HEAD_SUBCHUNK")) c->head_sub = atoll(e) >= 0 ? atoll(e) : c->head_sub;
  if (const char* e = getenv("OVN_HEAD_STREAMS")) c->head_streams = atoi(e) == 2 ? 2 : 1;
  if (const char* e = getenv("OVN_YAW_SIDE")) c->head_yaw_side = atoi(e) ? 1 : 0;
  int rc = ovn_spectral_prepare(c, nullptr);
  if (rc) {
    ovn_conv_release(&c->dft);
    if (c->tw64) (void)hipFree(c->tw64);
    delete c;
    return rc;
  }
  *out = c;
  return OVN_OK;
}

int ovn_destroy(ovn_ctx* ctx) {
  if (!ctx) return OVN_OK;
  if (ctx->comm) (void)ovn_comm_destroy(ctx);
  OVN_ON_DEVICE(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto& l : ctx->leg) ovn_conv_release(&l);
  ctx->head.release();
  ovn_conv_release(&ctx->dft);
  if (ctx->tw64) (void)hipFree(ctx->tw64);
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->norm_buf) (void)hipFree(ctx->norm_buf);
  if (ctx->actmax) (void)hipFree(ctx->actmax);
  if (ctx->c3_arrived) (void)hipFree(ctx->c3_arrived);
  if (ctx->seg_dev) (void)hipFree(ctx->seg_dev);
  if (ctx->seg_host) (void)hipHostFree(ctx->seg_host);
  if (ctx->seg_ev) (void)hipEventDestroy(ctx->seg_ev);
  if (ctx->seg_done) (void)hipEventDestroy(ctx->seg_done);
  if (ctx->aux_ready) {
    for (int i = 0; i < 2; ++i) {
      (void)hipStreamDestroy(ctx->aux[i]);
      (void)hipEventDestroy(ctx->ev_join[i]);
    }
    (void)hipEventDestroy(ctx->ev_fork);
  }
  delete ctx;
  return OVN_OK;
}

// Every device copy a leg layer keeps of its weights: the fp32 fragments + bias, the f16x3 fragments, and the kernel as registered
// (the data gradient of ovn_leg_backward reads it).  On failure nothing is left allocated.
static int leg_layer_prepare(OvnConvLayer* L, const float* kernel_dev, const float* bias_dev, hipStream_t stream) {
  int rc = ovn_conv_prepare(L, kernel_dev, bias_dev, stream);
  if (rc == OVN_OK) rc = ovn_conv_prepare_f16x3(L, kernel_dev, stream);
  if (rc == OVN_OK) {
    const size_t bytes = (size_t)L->kh * L->kw * L->cin * L->cout * sizeof(float);
    hipError_t e = hipMalloc((void**)&L->wraw, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(L->wraw, kernel_dev, bytes, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      ovn_set_error("layer %s: keeping the raw kernel failed: %s", L->name.c_str(), hipGetErrorString(e));
      rc = OVN_ERR_HIP;
    }
  }
  if (rc) ovn_conv_release(L);
  return rc;
}

int ovn_add_leg_layer(ovn_ctx* ctx, const char* name, const float* kernel_dev, const float* bias_dev, int kh, int kw,
                      int cin, int cout, int stride_h, int stride_w, void* stream) {
  OVN_REQUIRE(ctx && name && kernel_dev && bias_dev, OVN_ERR_ARG, "ovn_add_leg_layer: NULL argument");
  OVN_REQUIRE(kh > 0 && kw > 0 && cin > 0 && cout > 0 && stride_h > 0 && stride_w > 0, OVN_ERR_ARG,
              "ovn_add_leg_layer(%s): bad geometry", name);
  OVN_REQUIRE(!ctx->finalized, OVN_ERR_STATE, "ovn_add_leg_layer(%s): context already finalized", name);
  const int expect_cin = ctx->leg.empty() ? ctx->in_c : ctx->leg.back().cout;
  OVN_REQUIRE(cin == expect_cin, OVN_ERR_ARG, "ovn_add_leg_layer(%s): cin=%d but previous layer produces %d", name, cin, expect_cin);
  OVN_ON_DEVICE(ctx->device);
  OvnConvLayer L;
  L.name = name;
  L.kh = kh;
  L.kw = kw;
  L.cin = cin;
  L.cout = cout;
  L.sh = stride_h;
  L.sw = stride_w;
  L.relu = 1;  // every leg layer is Conv2D(..., activation='relu'), generateNet.py:161-214
  int rc = leg_layer_prepare(&L, kernel_dev, bias_dev, (hipStream_t)stream);
  if (rc) return rc;
  ctx->leg.push_back(L);
  return OVN_OK;
}

int ovn_set_leg_layer_weights(ovn_ctx* ctx, int layer, const float* kernel_dev, const float* bias_dev, void* stream) {
  OVN_REQUIRE(ctx && kernel_dev && bias_dev, OVN_ERR_ARG, "ovn_set_leg_layer_weights: NULL argument");
  OVN_REQUIRE(ctx->finalized, OVN_ERR_STATE, "ovn_set_leg_layer_weights: context not finalized");
  OVN_REQUIRE(layer >= 0 && layer < (int)ctx->leg.size(), OVN_ERR_ARG, "ovn_set_leg_layer_weights: no such leg layer %d", layer);
  OVN_ON_DEVICE(ctx->device);
  OvnConvLayer N = ctx->leg[layer];       // geometry; the new copies are built beside the old ones, which stay valid on failure
  N.wp = N.bias = N.wraw = nullptr;
  N.wp_h = N.wp_h16 = nullptr;
  N.sw_h = 1.f;
  int rc = leg_layer_prepare(&N, kernel_dev, bias_dev, (hipStream_t)stream);   // synchronises `stream`
  if (rc) return rc;
  ovn_conv_release(&ctx->leg[layer]);     // hipFree waits for whatever still reads the old copies
  ctx->leg[layer] = N;
  return OVN_OK;
}

void OvnHeadWeights::release() {
  ovn_conv_release(&c2);
  ovn_conv_release(&c3);
  for (void* p : {(void*)w1p, (void*)b1, w1p_h, w2p_h, (void*)w1raw, (void*)w1sum, (void*)w1col, wsp_h, (void*)w2sum, w1p_b3, w2p_b3,
                  (void*)w2raw, (void*)w3raw, (void*)wd, (void*)bd})
    if (p) (void)hipFree(p);
  *this = OvnHeadWeights();
}

// a device copy of n floats registered with the head
static int head_keep(float** dst, const float* src, size_t n, hipStream_t stream) {
  OVN_HIP_CHECK(hipMalloc((void**)dst, n * sizeof(float)));
  OVN_HIP_CHECK(hipMemcpyAsync(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
  return OVN_OK;
}

static OvnConvLayer head_conv(const char* name, int kh, int kw, int cin, int cout, int sh) {
  OvnConvLayer L;
  L.name = name;
  L.kh = kh;
  L.kw = kw;
  L.cin = cin;
  L.cout = cout;
  L.sh = sh;
  L.sw = 1;
  L.relu = 1;
  return L;
}

// Every copy of a head weight set for conv1size hs and hg column groups into the (empty) set N; synchronises `stream`.  On failure N
// holds whatever was allocated so far: the caller releases it.
static int head_weights_prepare(OvnHeadWeights* N, int hs, int hg, const float* c1k, const float* c1b, const float* c2k, const float* c2b,
                                const float* c3k, const float* c3b, const float* dk, const float* db, hipStream_t stream) {
  const bool general = (hs != OVN_S);   // any other conv1size: general fp32 path (delta_head_generic.hip), no fast-path operands
  int rc = general ? head_keep(&N->w1raw, c1k, (size_t)hs * OVN_FEAT_C * OVN_C1_OUT, stream) : ovn_delta_prepare_w1(N, c1k, stream);
  if (rc == OVN_OK) rc = head_keep(&N->b1, c1b, OVN_C1_OUT, stream);
  // c_conv2 (15,1,64,128): as a GEMM operand it is the [960][128] matrix, k = di*64 + o
  N->c2 = head_conv("c_conv2", hs, 1, OVN_C1_OUT, OVN_C2_OUT, hs);
  if (rc == OVN_OK) rc = ovn_conv_prepare(&N->c2, c2k, c2b, stream);
  if (rc == OVN_OK && !general) rc = ovn_delta_prepare_f16x3(N, c1k, c1b, c2k, stream);
  N->c3 = head_conv("c_conv3", 3, 3, OVN_C2_OUT, OVN_C3_OUT, 1);
  if (rc == OVN_OK) rc = ovn_conv_prepare(&N->c3, c3k, c3b, stream);
  if (rc == OVN_OK && !general) rc = ovn_conv_prepare_f16x3(&N->c3, c3k, stream);
  // Keras-order copies for ovn_delta_head_grad: W3 always, W2 where the fast-path preparation above did not leave one
  if (rc == OVN_OK) rc = head_keep(&N->w3raw, c3k, (size_t)9 * OVN_C2_OUT * OVN_C3_OUT, stream);
  if (rc == OVN_OK && !N->w2raw) rc = head_keep(&N->w2raw, c2k, (size_t)hs * OVN_C1_OUT * OVN_C2_OUT, stream);
  if (rc == OVN_OK) rc = head_keep(&N->wd, dk, (size_t)(hg - 2) * (hg - 2) * OVN_C3_OUT, stream);   // 123904 at conv1size 15
  if (rc == OVN_OK) rc = head_keep(&N->bd, db, 1, stream);
  if (rc == OVN_OK) OVN_HIP_CHECK(hipStreamSynchronize(stream));
  return rc;
}

int ovn_set_head_weights(ovn_ctx* ctx, const float* c1k, const float* c1b, const float* c2k, const float* c2b,
                         const float* c3k, const float* c3b, const float* dk, const float* db, void* stream_) {
  OVN_REQUIRE(ctx && c1k && c1b && c2k && c2b && c3k && c3b && dk && db, OVN_ERR_ARG, "ovn_set_head_weights: NULL argument");
  OVN_ON_DEVICE(ctx->device);
  const int hg = ctx_feat_w(ctx) / ctx->head_s;   // G of the Dense kernel registered below
  OVN_REQUIRE(hg >= 3, OVN_ERR_ARG, "ovn_set_head_weights: conv1size %d leaves %d column groups, c_conv3 needs 3", ctx->head_s, hg);
  OvnHeadWeights N;   // the new set is built beside the one in use, which keeps serving (head_set unchanged) on failure
  const int rc = head_weights_prepare(&N, ctx->head_s, hg, c1k, c1b, c2k, c2b, c3k, c3b, dk, db, (hipStream_t)stream_);
  if (rc) {
    N.release();
    return rc;
  }
  ctx->head.release();   // hipFree waits for whatever still reads the old copies
  ctx->head = N;
  ctx->head_g = hg;
  ctx->head_set = true;
  return OVN_OK;
}

// Leg precision f16x3 at the context's input size: the first layer that falls to the generic kernel (neither the fused front or
// tail nor a strip kernel takes it) with fewer output positions per image than that kernel's tiles need
// (ovn_conv_forward_f16x3), or -1.  Known once the layers and the input size are: refused before the first ovn_leg.
static int leg_f16x3_unserved(const ovn_ctx* ctx) {
  int h = ctx->in_h, w = ctx->in_w;
  for (size_t li = 0; li < ctx->leg.size(); ++li) {
    const auto& l = ctx->leg[li];
    if (h < l.kh || w < l.kw) return -1;          // ovn_finalize refuses that itself
    const int oh = (h - l.kh) / l.sh + 1, ow = (w - l.kw) / l.sw + 1;
    if (li == 0 && ovn_leg_front_matches(ctx, li, h, w)) {
      const auto& l2 = ctx->leg[1];
      h = (oh - l2.kh) / l2.sh + 1;
      w = (ow - l2.kw) / l2.sw + 1;
      ++li;
      continue;
    }
    if (ovn_leg_tail_matches(ctx, li, h, w)) return -1;
    if (!ovn_conv_strip_matches(l, h, w) && (long long)oh * ow < 128) return (int)li;
    h = oh;
    w = ow;
  }
  return -1;
}

int ovn_finalize(ovn_ctx* ctx, int* feat_w) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_finalize: ctx is NULL");
  OVN_REQUIRE(!ctx->leg.empty(), OVN_ERR_STATE, "ovn_finalize: no leg layers registered");
  int h = ctx->in_h, w = ctx->in_w, c = ctx->in_c;
  for (const auto& l : ctx->leg) {
    OVN_REQUIRE(h >= l.kh && w >= l.kw, OVN_ERR_ARG, "ovn_finalize: layer %s does not fit its %dx%d input", l.name.c_str(), h, w);
    h = (h - l.kh) / l.sh + 1;
    w = (w - l.kw) / l.sw + 1;
    c = l.cout;
  }
  OVN_REQUIRE(h == 1 && w >= OVN_FEAT_W_MIN && w <= OVN_FEAT_W_MAX && c == OVN_FEAT_C, OVN_ERR_ARG,
              "ovn_finalize: leg produces %dx%dx%d, the heads need 1 x W x %d with %d <= W <= %d", h, w, c, OVN_FEAT_C, OVN_FEAT_W_MIN,
              OVN_FEAT_W_MAX);
  OVN_REQUIRE(!ctx->head_set || w / ctx->head_s == ctx->head_g, OVN_ERR_STATE,
              "ovn_finalize: leg width %d gives %d column groups, the head weights were registered for %d", w, w / ctx->head_s,
              ctx->head_g);
  if (ctx->leg_mode != 0) {
    const int bad = leg_f16x3_unserved(ctx);
    OVN_REQUIRE(bad < 0, OVN_ERR_ARG,
                "ovn_finalize: layer %s: fewer than 128 output positions per image in leg precision f16x3 (ovn_set_leg_precision(ctx, 0) "
                "before ovn_finalize runs this leg in fp32)", ctx->leg[bad < 0 ? 0 : bad].name.c_str());
  }
  ctx->feat_w = w;
  ctx->finalized = true;
  if (feat_w) *feat_w = w;
  return OVN_OK;
}

int ovn_leg(ovn_ctx* ctx, const float* images_dev, int64_t n, float* features_dev, void* stream_) {
  OVN_REQUIRE(ctx && ctx->finalized, OVN_ERR_STATE, "ovn_leg: context not finalized");
  OVN_REQUIRE(n >= 0, OVN_ERR_ARG, "ovn_leg: n < 0");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(images_dev && features_dev, OVN_ERR_ARG, "ovn_leg: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  // largest intermediate activation per scan decides the ping-pong buffer size
  size_t max_act = 0;
  {
    int h = ctx->in_h, w = ctx->in_w;
    for (const auto& l : ctx->leg) {
      h = (h - l.kh) / l.sh + 1;
      w = (w - l.kw) / l.sw + 1;
      const size_t e = (size_t)h * w * l.cout;
      if (e > max_act) max_act = e;
    }
  }
  // process the batch in slices so the scratch stays bounded (2 x slice x 770 KB at C=4: at most 1.6 GB); the slices are BALANCED
  // (1025 scans = 513 + 512, not 1024 + 1: a one-scan slice costs a fifth of a 256-scan one, its kernels being a handful of
  // workgroups deep in their own latency) -- a scan's result does not depend on the slice it falls into.  Slices of 256 / 512 / 1024
  // scans: 5.18 / 5.00 / 4.93 ms per 1025 scans (fewer launch ramps and drains between the five kernels of a slice)
  const int64_t nslices = (n + OVN_LEG_SLICE - 1) / OVN_LEG_SLICE;
  const int64_t slice = (n + nslices - 1) / nslices;
  LegScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)slice * max_act, 2, (size_t)0, (size_t)0);
  if (rc) return rc;
  float* const* buf = sc.buf;
  const size_t in_elems = (size_t)ctx->in_h * ctx->in_w * ctx->in_c;
  const size_t feat_elems = (size_t)ctx->feat_w * OVN_FEAT_C;
  OVN_REQUIRE(ctx->leg.size() + 1 <= OVN_ACTMAX_SLOTS, OVN_ERR_STATE, "ovn_leg: too many leg layers");
  const size_t actmax_bytes = (size_t)OVN_ACTMAX_SLOTS * OVN_LEG_SLICE * OVN_ACTMAX_STRIDE * sizeof(unsigned);
  if (ctx->leg_mode != 0 && !ctx->actmax) OVN_HIP_CHECK(hipMalloc((void**)&ctx->actmax, actmax_bytes));
  for (int64_t s0 = 0; s0 < n; s0 += slice) {
    const int nb = (int)((n - s0 < slice) ? (n - s0) : slice);
    const float* cur = images_dev + (size_t)s0 * in_elems;
    int h = ctx->in_h, w = ctx->in_w;
    if (ctx->leg_mode != 0) {
      // f16x3: word [li][scan of the slice] (rows of `slice` words: a one-scan call clears 12 words, not 12 x 1024) = max |input of
      // layer li| of that scan, folded by the kernel that produces it.  Scales are per scan
      // and every call size runs the same kernels, so a scan's feature volume does not depend on the batch it is computed in
      // (the first layer's kernel at C = 4 and the fused tail take the maximum of their own strip / tile instead)
      OVN_HIP_CHECK(hipMemsetAsync(ctx->actmax, 0, (ctx->leg.size() + 1) * (size_t)slice * OVN_ACTMAX_STRIDE * sizeof(unsigned), stream));
      const bool own = (reinterpret_cast<uintptr_t>(cur) & 15) == 0 && ovn_conv_strip_own_scale(ctx->leg[0], h, w);
      if (!own) {
        OvnProfScope ps(ctx, OVN_K_LEG, stream);
        rc = ovn_absmax_forward(cur, nb, (long long)in_elems, ctx->actmax, stream);
        if (rc) return rc;
      }
    }
    for (size_t li = 0; li < ctx->leg.size(); ++li) {
      const bool last = (li + 1 == ctx->leg.size());
      float* dst = last ? features_dev + (size_t)s0 * feat_elems : buf[li & 1];
      int oh = 0, ow = 0;
      // f16x3, C = 4: s_conv1 + s_conv2 as one kernel (the activation between them never leaves the CU)
      if (ctx->leg_mode != 0 && li == 0 && (reinterpret_cast<uintptr_t>(cur) & 15) == 0 && ovn_leg_front_matches(ctx, li, h, w)) {
        OvnProfScope ps(ctx, OVN_K_LEG, stream);
        float* dst2 = buf[(li + 1) & 1];
        rc = ovn_leg_front_forward(ctx, li, cur, nb, h, w, dst2, &oh, &ow, ctx->actmax + (li + 2) * (size_t)slice * OVN_ACTMAX_STRIDE, stream);
        if (rc) return rc;
        cur = dst2;
        h = oh;
        w = ow;
        ++li;          // two layers done
        continue;
      }
      // f16x3: the six 1 x KW layers at the end run as one kernel with the activations kept in LDS
      if (ctx->leg_mode != 0 && ovn_leg_tail_matches(ctx, li, h, w)) {
        OvnProfScope ps(ctx, OVN_K_LEG, stream);
        rc = ovn_leg_tail_forward(ctx, li, cur, nb, w, features_dev + (size_t)s0 * feat_elems, stream);
        if (rc) return rc;
        break;
      }
      {
        OvnProfScope ps(ctx, OVN_K_LEG, stream);
        rc = (ctx->leg_mode == 0) ? ovn_conv_forward(ctx->leg[li], cur, nb, h, w, dst, &oh, &ow, stream)
                                  : ovn_conv_forward_f16x3(ctx->leg[li], cur, nb, h, w, dst, &oh, &ow, ctx->actmax + li * (size_t)slice * OVN_ACTMAX_STRIDE,
                                                           last ? nullptr : ctx->actmax + (li + 1) * (size_t)slice * OVN_ACTMAX_STRIDE, stream);
      }
      if (rc) return rc;
      cur = dst;
      h = oh;
      w = ow;
    }
  }
  return OVN_OK;
}

// ---- training the legs (leg_backward.hip) ---------------------------------------------------------------------------------------
// per layer: input height / width and elements per scan of its output
struct LegGeom {
  std::vector<int> h, w;
  std::vector<int64_t> act;
  int64_t act_total = 0, act_max = 0, params = 0;
};

static LegGeom leg_geom(const ovn_ctx* ctx) {
  LegGeom g;
  int h = ctx->in_h, w = ctx->in_w;
  for (const auto& l : ctx->leg) {
    g.h.push_back(h);
    g.w.push_back(w);
    h = (h - l.kh) / l.sh + 1;
    w = (w - l.kw) / l.sw + 1;
    g.act.push_back((int64_t)h * w * l.cout);
    g.act_total += g.act.back();
    g.act_max = std::max(g.act_max, g.act.back());
    g.params += (int64_t)l.kh * l.kw * l.cin * l.cout + l.cout;
  }
  return g;
}

int ovn_leg_layer_count(ovn_ctx* ctx, int* layers) {
  OVN_REQUIRE(ctx && layers, OVN_ERR_ARG, "ovn_leg_layer_count: NULL argument");
  *layers = (int)ctx->leg.size();
  return OVN_OK;
}

int ovn_leg_param_sizes(ovn_ctx* ctx, int64_t* sizes) {
  OVN_REQUIRE(ctx && sizes, OVN_ERR_ARG, "ovn_leg_param_sizes: NULL argument");
  for (size_t li = 0; li < ctx->leg.size(); ++li) {
    const auto& l = ctx->leg[li];
    sizes[2 * li] = (int64_t)l.kh * l.kw * l.cin * l.cout;
    sizes[2 * li + 1] = l.cout;
  }
  return OVN_OK;
}

int ovn_leg_activation_sizes(ovn_ctx* ctx, int64_t* sizes) {
  OVN_REQUIRE(ctx && sizes, OVN_ERR_ARG, "ovn_leg_activation_sizes: NULL argument");
  OVN_REQUIRE(ctx->finalized, OVN_ERR_STATE, "ovn_leg_activation_sizes: context not finalized");
  const LegGeom g = leg_geom(ctx);
  for (size_t li = 0; li < g.act.size(); ++li) sizes[li] = g.act[li];
  return OVN_OK;
}

int ovn_leg_forward_train(ovn_ctx* ctx, const float* images_dev, int64_t n, float* acts_dev, void* stream_) {
  OVN_REQUIRE(ctx && images_dev && acts_dev, OVN_ERR_ARG, "ovn_leg_forward_train: NULL argument");
  OVN_REQUIRE(n >= 1 && n < (1ll << 31), OVN_ERR_ARG, "ovn_leg_forward_train: bad n %lld", (long long)n);
  OVN_REQUIRE(ctx->finalized, OVN_ERR_STATE, "ovn_leg_forward_train: context not finalized");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const LegGeom g = leg_geom(ctx);
  const float* cur = images_dev;
  float* dst = acts_dev;
  for (size_t li = 0; li < ctx->leg.size(); ++li) {
    OvnProfScope ps(ctx, OVN_K_LEG, stream);
    int oh = 0, ow = 0;
    int rc = ovn_conv_forward(ctx->leg[li], cur, (int)n, g.h[li], g.w[li], dst, &oh, &ow, stream);
    if (rc) return rc;
    cur = dst;
    dst += (size_t)n * g.act[li];
  }
  return OVN_OK;
}

int ovn_leg_backward(ovn_ctx* ctx, const float* images_dev, const float* acts_dev, int64_t n, const float* dfeat_dev, float* grad_dev,
                     int64_t slice_scans, void* stream_) {
  OVN_REQUIRE(ctx && images_dev && acts_dev && dfeat_dev && grad_dev, OVN_ERR_ARG, "ovn_leg_backward: NULL argument");
  OVN_REQUIRE(n >= 1 && n < (1ll << 31), OVN_ERR_ARG, "ovn_leg_backward: bad n %lld", (long long)n);
  OVN_REQUIRE(slice_scans >= 0, OVN_ERR_ARG, "ovn_leg_backward: slice_scans %lld < 0", (long long)slice_scans);
  OVN_REQUIRE(ctx->finalized, OVN_ERR_STATE, "ovn_leg_backward: context not finalized");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const LegGeom g = leg_geom(ctx);
  const int L = (int)ctx->leg.size();
  constexpr int64_t SB = OVN_LEG_GRAD_SCAN_BLOCK;
  int64_t slice = slice_scans == 0 ? 8 * SB : std::max<int64_t>(SB, slice_scans / SB * SB);
  slice = std::min(slice, std::min<int64_t>((n + SB - 1) / SB * SB, 65535 / SB * SB));
  const int nmax = (int)std::min(slice, n);
  size_t part_bytes = 0;
  for (int li = 0; li < L; ++li) part_bytes = std::max(part_bytes, ovn_leg_grad_part_bytes(ctx->leg[li], g.h[li], g.w[li], nmax));
  LegScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)nmax * g.act_max, 2, (size_t)g.params, part_bytes);
  if (rc) return rc;
  scratch_overwritten(ctx);
  float* const* buf = sc.buf;
  double *acc = sc.acc, *part = sc.part;
  OVN_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)g.params * sizeof(double), stream));
  std::vector<int64_t> act_off(L, 0), par_off(L, 0);
  for (int li = 1; li < L; ++li) {
    act_off[li] = act_off[li - 1] + g.act[li - 1];
    par_off[li] = par_off[li - 1] + (int64_t)ctx->leg[li - 1].K * ctx->leg[li - 1].cout + ctx->leg[li - 1].cout;
  }
  const size_t in_elems = (size_t)ctx->in_h * ctx->in_w * ctx->in_c;
  for (int64_t s0 = 0; s0 < n; s0 += slice) {
    const int nb = (int)std::min(slice, n - s0);
    OvnProfScope ps(ctx, OVN_K_LEG, stream);
    int cur = 0;
    rc = ovn_leg_mask_forward(dfeat_dev + (size_t)s0 * g.act[L - 1], acts_dev + (size_t)n * act_off[L - 1] + (size_t)s0 * g.act[L - 1],
                              buf[cur], (long long)nb * g.act[L - 1], stream);
    if (rc) return rc;
    for (int li = L - 1; li >= 0; --li) {
      const auto& l = ctx->leg[li];
      const float* x = li ? acts_dev + (size_t)n * act_off[li - 1] + (size_t)s0 * g.act[li - 1] : images_dev + (size_t)s0 * in_elems;
      double* ak = acc + par_off[li];
      // nothing trains upstream of the leg: the data gradient stops at the input of layer 1
      rc = ovn_leg_layer_backward(l, x, buf[cur], nb, g.h[li], g.w[li], li ? buf[cur ^ 1] : nullptr, li ? x : nullptr, ak,
                                  ak + (int64_t)l.K * l.cout, part, stream);
      if (rc) return rc;
      cur ^= 1;
    }
  }
  return ovn_leg_grad_round(acc, grad_dev, g.params, stream);
}

int ovn_debug_conv_grad(ovn_ctx* ctx, int layer, const float* in_dev, const float* out_dev, const float* dout_dev, int nb, int h, int w,
                        float* din_dev, float* dkernel_dev, float* dbias_dev, void* stream_) {
  OVN_REQUIRE(ctx && in_dev && out_dev && dout_dev, OVN_ERR_ARG, "ovn_debug_conv_grad: NULL argument");
  OVN_REQUIRE(layer >= 0 && layer < (int)ctx->leg.size(), OVN_ERR_ARG, "ovn_debug_conv_grad: no such leg layer %d", layer);
  OVN_REQUIRE(nb >= 1 && nb <= 65535, OVN_ERR_ARG, "ovn_debug_conv_grad: bad nb %d", nb);
  const OvnConvLayer& l = ctx->leg[layer];
  OVN_REQUIRE(h >= l.kh && w >= l.kw, OVN_ERR_ARG, "ovn_debug_conv_grad: input %dx%d smaller than the kernel of %s", h, w, l.name.c_str());
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int oh = (h - l.kh) / l.sh + 1, ow = (w - l.kw) / l.sw + 1;
  const long long out_elems = (long long)nb * oh * ow * l.cout;
  const int64_t kelems = (int64_t)l.K * l.cout;
  LegScratch sc;
  int rc = ovn_ws_layout(ctx, stream, &sc, (size_t)out_elems, 1, (size_t)(kelems + l.cout), ovn_leg_grad_part_bytes(l, h, w, nb));
  if (rc) return rc;
  scratch_overwritten(ctx);
  float* dym = sc.buf[0];
  double *acc = sc.acc, *part = sc.part;
  OVN_HIP_CHECK(hipMemsetAsync(acc, 0, (size_t)(kelems + l.cout) * sizeof(double), stream));
  OvnProfScope ps(ctx, OVN_K_LEG, stream);
  rc = ovn_leg_mask_forward(dout_dev, out_dev, dym, out_elems, stream);
  if (rc) return rc;
  rc = ovn_leg_layer_backward(l, in_dev, dym, nb, h, w, din_dev, nullptr, dkernel_dev ? acc : nullptr, dbias_dev ? acc + kelems : nullptr,
                              part, stream);
  if (rc) return rc;
  if (dkernel_dev) rc = ovn_leg_grad_round(acc, dkernel_dev, kelems, stream);
  if (rc == OVN_OK && dbias_dev) rc = ovn_leg_grad_round(acc + kelems, dbias_dev, l.cout, stream);
  return rc;
}

int ovn_corr_head(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                  int64_t n, int32_t* yaw, float* corr, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_corr_head: ctx is NULL");
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_corr_head: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_l && feats_r && yaw, OVN_ERR_ARG, "ovn_corr_head: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_CORR, (hipStream_t)stream);
  return ovn_corr_forward(feats_l, lidx, feats_r, ridx, (int)n, ctx_feat_w(ctx), yaw, corr, (hipStream_t)stream, ctx->corr_norm);
}

int ovn_spectrum(ovn_ctx* ctx, const float* feats_dev, int64_t n, float* spectra_dev, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_spectrum: ctx is NULL");
  OVN_REQUIRE(ctx_feat_w(ctx) == OVN_FEAT_W, OVN_ERR_ARG,
              "ovn_spectrum: the spectral correlation head needs 360-column feature volumes (the leg produces %d)", ctx_feat_w(ctx));
  OVN_REQUIRE(n >= 0 && n < (1ll << 24), OVN_ERR_ARG, "ovn_spectrum: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_dev && spectra_dev, OVN_ERR_ARG, "ovn_spectrum: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_SPECTRUM, (hipStream_t)stream);
  return ovn_spectrum_forward(ctx, feats_dev, (int)n, spectra_dev, (hipStream_t)stream);
}

int ovn_corr_head_spectral(ovn_ctx* ctx, const float* spec_l, const int32_t* lidx, const float* spec_r,
                           const int32_t* ridx, int64_t n, int32_t* yaw, float* corr, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_corr_head_spectral: ctx is NULL");
  OVN_REQUIRE(ctx_feat_w(ctx) == OVN_FEAT_W, OVN_ERR_ARG,
              "ovn_corr_head_spectral: the spectral correlation head needs 360-column feature volumes (the leg produces %d)", ctx_feat_w(ctx));
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_corr_head_spectral: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(spec_l && spec_r && yaw, OVN_ERR_ARG, "ovn_corr_head_spectral: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_CORR_SPECTRAL, (hipStream_t)stream);
  return ovn_corr_spectral_forward(ctx, spec_l, lidx, spec_r, ridx, (int)n, yaw, corr, (hipStream_t)stream);
}

// ---- side streams of a head call -----------------------------------------------------------------------------------------------
// A head call may spread its launches over the caller's stream and two context-owned side streams: the HBM-bound yaw head next to
// the matrix-core-bound Delta kernels, and the sub-chunks of a sweep alternating between two streams so that the prepare / c_conv2 /
// c_conv3 kernels of one sub-chunk run beside the contraction kernel of the next.  Fork and join are events on the caller's stream:
// to the caller the call still behaves as if everything had been enqueued on `stream`.
static int head_streams_ready(ovn_ctx* ctx) {
  if (ctx->aux_ready) return OVN_OK;
  for (int i = 0; i < 2; ++i) {
    OVN_HIP_CHECK(hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking));
    OVN_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming));
  }
  OVN_HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  ctx->aux_ready = true;
  return OVN_OK;
}

struct OvnFork {   // fork on construction-time request, join (on every exit path) in the destructor
  ovn_ctx* ctx;
  hipStream_t stream;
  bool used[2] = {false, false};
  bool forked = false;
  OvnFork(ovn_ctx* c, hipStream_t s) : ctx(c), stream(s) {}
  int fork() {
    if (forked) return OVN_OK;
    int rc = head_streams_ready(ctx);
    if (rc) return rc;
    OVN_HIP_CHECK(hipEventRecord(ctx->ev_fork, stream));
    forked = true;
    return OVN_OK;
  }
  // side stream i, ordered behind everything the caller had enqueued on `stream` when fork() ran
  int side(int i, hipStream_t* out) {
    int rc = fork();
    if (rc) return rc;
    if (!used[i]) {
      OVN_HIP_CHECK(hipStreamWaitEvent(ctx->aux[i], ctx->ev_fork, 0));
      used[i] = true;
    }
    *out = ctx->aux[i];
    return OVN_OK;
  }
  int join() {
    int rc = OVN_OK;
    for (int i = 0; i < 2; ++i)
      if (used[i]) {
        used[i] = false;
        if (hipEventRecord(ctx->ev_join[i], ctx->aux[i]) != hipSuccess || hipStreamWaitEvent(stream, ctx->ev_join[i], 0) != hipSuccess) {
          ovn_set_error("joining the head's side stream failed");
          rc = OVN_ERR_HIP;
        }
      }
    return rc;
  }
  ~OvnFork() { (void)join(); }
};

// The fp32 routes of a head call: the fused MFMA kernel of delta_head.hip at conv1size 15 (any width; with ovn_set_head_width_split,
// head mode 1 takes the f16x3 kernels of delta_head_w_f16x3.hip inside ovn_delta_forward at widths other than 360), the general
// kernels of delta_head_generic.hip at any other conv1size.  Chunked so that the scratch stays near 2 GB and within head_chunk pairs.
static int delta_head_run_f32(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                              int64_t n, float* overlap, float* logit, int32_t* yaw, float* corr, int corr_mode, const float* spec_l,
                              const float* spec_r, hipStream_t stream) {
  const int fw = ctx_feat_w(ctx);
  const size_t feat_elems = (size_t)fw * OVN_FEAT_C;
  OVN_REQUIRE(corr_mode != 2 || fw == OVN_FEAT_W, OVN_ERR_ARG, "spectral correlation head at feature width %d", fw);
  const bool fusedc12 = (ctx->head_s == OVN_S);
  const size_t pb = fusedc12 ? ovn_delta_pair_bytes(ctx->head_g) : ovn_delta_generic_pair_bytes(fw, ctx->head_g);
  int64_t chunk = (int64_t)((2ull << 30) / pb);
  chunk = chunk < 1 ? 1 : (chunk > 1024 ? 1024 : chunk);
  if (ctx->head_chunk < chunk) chunk = ctx->head_chunk;
  const int64_t cmax = n < chunk ? n : chunk;
  OvnDeltaF32Scratch sc;        // one chunk of either route
  OvnDeltaGenericScratch gsc;
  int rc = fusedc12 ? ovn_ws_layout(ctx, stream, &sc, cmax, ctx->head_g, ctx->head_width_split && ctx->head_mode == 1)
                    : ovn_ws_layout(ctx, stream, &gsc, cmax, fw, ctx->head_g);
  if (rc) return rc;
  scratch_overwritten(ctx);
  OvnFork fk(ctx, stream);
  if (corr_mode == 2) {   // ONE launch for all n pairs, beside the Delta kernels when the pipeline asks for a side stream
    hipStream_t ys = stream;
    if (ctx->head_yaw_side) {
      rc = fk.side(1, &ys);
      if (rc) return rc;
    }
    OvnProfScope ps(ctx, OVN_K_CORR_SPECTRAL, ys);
    rc = ovn_corr_spectral_forward(ctx, spec_l, lidx, spec_r, ridx, (int)n, yaw, corr, ys);
    if (rc) return rc;
  }
  for (int64_t p0 = 0; p0 < n; p0 += chunk) {
    const int np = (int)((n - p0 < chunk) ? (n - p0) : chunk);
    const float* fl = lidx ? feats_l : feats_l + (size_t)p0 * feat_elems;
    const int32_t* li = lidx ? lidx + p0 : nullptr;
    const int32_t* ri = ridx ? ridx + p0 : nullptr;
    if (corr_mode == 1) {
      OvnProfScope ps(ctx, OVN_K_CORR, stream);
      rc = ovn_corr_forward(fl, li, feats_r, ri, np, fw, yaw + p0, corr ? corr + (size_t)p0 * fw : nullptr, stream, ctx->corr_norm);
      if (rc) return rc;
    }
    if (fusedc12) {   // times its Delta, c_conv3 and Dense kernels separately
      rc = ovn_delta_forward(ctx, fl, li, feats_r, ri, np, sc, overlap + p0, logit ? logit + p0 : nullptr, stream);
    } else {
      OvnProfScope ps(ctx, OVN_K_DELTA, stream);
      rc = ovn_delta_generic_forward(ctx, fl, li, feats_r, ri, np, gsc, overlap + p0, logit ? logit + p0 : nullptr, stream);
    }
    if (rc) return rc;
  }
  if (fusedc12 && n > 0 && n <= chunk) {   // one chunk: its o2 / o3 regions hold every pair for the test hook
    ctx->dbg_o2 = sc.o2;
    ctx->dbg_o3 = sc.o3;
    ctx->dbg_n = n;
  }
  return fk.join();
}

// Scratch of a split-operand head call (f16x3 / bf16x3 at 360 columns): o2 of a chunk | o3 of the chunk (bf16x3) or its Dense partials
// (f16x3) | nsub blocks of sub_bytes, sub-chunk j's OvnDeltaSubScratch in block j | the segment state of a segmented pass
struct HeadScratch {
  float *o2 = nullptr, *o3 = nullptr;
  char* sub = nullptr;
  size_t sub_bytes = 0;
  OvnDeltaSegScratch seg;
  HeadScratch() = default;
  HeadScratch(OvnCarver& c, int64_t cmax, bool fused, int64_t sub_pairs, int nsub, bool per_pair_right, int nseg) {
    o2 = c.take<float>((size_t)cmax * OVN_G * OVN_G * OVN_C2_OUT);
    o3 = c.take<float>((size_t)cmax * (fused ? OVN_DENSE_PARTIALS : OVN_DENSE_IN));
    sub_bytes = ovn_delta_f16x3_scratch_bytes((int)sub_pairs, per_pair_right);
    sub = c.take<char>(sub_bytes * nsub);
    if (nseg) seg = OvnDeltaSegScratch(c, nseg);
  }
  // the block of sub-chunk j, laid out for its np <= sub_pairs pairs
  OvnDeltaSubScratch sub_chunk(int j, int np, bool per_pair_right) const {
    OvnCarver c(sub + (size_t)j * sub_bytes);
    return OvnDeltaSubScratch(c, np, per_pair_right);
  }
};

// Delta (overlap) head on n pairs [+ one of the correlation heads]; shared by ovn_heads, ovn_delta_head and ovn_heads_spectral.
//   corr_mode 0: none; 1: direct form on the feature volumes (per chunk, on the caller's stream, as ovn_heads always did);
//             2: spectral form on (spec_l, spec_r): ONE launch for all n pairs on a side stream, beside the Delta kernels.
// conv1size != 15, W != 360 or head mode 0 run the fp32 routes above.  The split-operand modes (360 columns) follow: the sweep is cut
// into chunks of <= ctx->head_chunk pairs (the scratch is sized for one chunk) and every chunk into sub-chunks of ctx->head_sub pairs
// that alternate between ctx->head_streams streams (sub-chunk j of every chunk uses scratch region j and stream j % streams, so a
// region is only ever reused in stream order).
static int delta_head_run(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r,
                          const int32_t* ridx, int64_t n, float* overlap, float* logit, int32_t* yaw, float* corr,
                          int corr_mode, const float* spec_l, const float* spec_r, const float* dcache_l, hipStream_t stream,
                          const OvnSegPass* seg = nullptr) {   // seg: a pass of ovn_heads_segments (f16x3 fused path only)
  ctx->dbg_live = nullptr;   // ovn_head_walk_stats describes THIS call (a sweep that compacts sets it again)
  const int fw = ctx_feat_w(ctx);
  if (ctx->head_s != OVN_S || fw != OVN_FEAT_W || ctx->head_mode == 0)
    return delta_head_run_f32(ctx, feats_l, lidx, feats_r, ridx, n, overlap, logit, yaw, corr, corr_mode, spec_l, spec_r, stream);
  const size_t feat_elems = (size_t)fw * OVN_FEAT_C;
  const size_t o2_elems = (size_t)OVN_G * OVN_G * OVN_C2_OUT;   // 24*24*128 per pair
  const size_t o3_elems = (size_t)OVN_DENSE_IN;                 // 22*22*256 per pair
  // head modes: 1 = f16x3 (prepare / contraction / c_conv2 kernels, fused c_conv3 + Dense); 2 = bf16x3 (the same three Delta kernels
  // with the exact bf16 split, generic fp32 c_conv3, Dense)
  const bool fused = (ctx->head_mode == 1);
  const int64_t chunk = ctx->head_chunk;                        // pairs per pass over the scratch (f16x3: 3.2 MB per pair)
  const int64_t cmax = n < chunk ? n : chunk;
  // sub-chunks (a segmented pass keeps one: its per-segment query state is shared by all of its pairs)
  int64_t sub = (!seg && ctx->head_sub > 0 && ctx->head_sub < cmax) ? ctx->head_sub : cmax;
  const int nsub_max = (int)((cmax + sub - 1) / sub);
  const int nstreams = (nsub_max > 1 && ctx->head_streams > 1) ? 2 : 1;
  // second scratch region: o3 (n,22,22,256) in bf16x3 mode; in f16x3 mode c_conv3 and the Dense layer are one kernel and only
  // OVN_DENSE_PARTIALS partial sums per pair (band x half of the output channels x half of the m-tiles) leave it.  Then per-pair
  // scales, packed volumes, linear terms and the c_conv1 rows between the two Delta kernels (2.9 MB per pair), one self-contained
  // block per sub-chunk
  HeadScratch hs;
  int rc = ovn_ws_layout(ctx, stream, &hs, cmax, fused, sub, nsub_max, ridx != nullptr, seg ? seg->nseg : 0);
  if (rc) return rc;
  if (fused && ctx->c3_arrived_n < chunk) {   // arrival counters of the fused c_conv3 + Dense kernel, one per pair of a chunk (sized
    OVN_HIP_CHECK(hipStreamSynchronize(stream));   // by the chunk, not by this call: a growing sweep must not re-allocate): zeroed
    if (ctx->c3_arrived) (void)hipFree(ctx->c3_arrived);   // once, left zeroed by every launch
    ctx->c3_arrived = nullptr;
    ctx->c3_arrived_n = 0;
    OVN_HIP_CHECK(hipMalloc((void**)&ctx->c3_arrived, (size_t)chunk * sizeof(unsigned)));
    OVN_HIP_CHECK(hipMemsetAsync(ctx->c3_arrived, 0, (size_t)chunk * sizeof(unsigned), stream));
    ctx->c3_arrived_n = chunk;
  }
  float *o2 = hs.o2, *o3 = hs.o3;
  ctx->dbg_o2max = nullptr;
  ctx->dbg_o2 = o2;
  ctx->dbg_o3 = fused ? nullptr : o3;
  ctx->dbg_partial = fused ? o3 : nullptr;
  ctx->dbg_n = sub < cmax ? sub : cmax;      // the activations of the first sub-chunk stay addressable for the tests

  OvnFork fk(ctx, stream);
  bool a2_in_yaw = false;
  if (corr_mode == 2) {
    hipStream_t ys = stream;
    if (ctx->head_yaw_side) {
      rc = fk.side(1, &ys);
      if (rc) return rc;
    }
    OvnProfScope ps(ctx, OVN_K_CORR_SPECTRAL, ys);
    // a small 1-vs-N sweep in one sub-chunk: the query's right-volume term of the Delta head rides in the yaw launch (csrc/delta_a2.h)
    a2_in_yaw = ridx == nullptr && n <= OVN_A2_IN_YAW_MAX_PAIRS && n <= chunk && ys == stream && nsub_max == 1;
    rc = ovn_corr_spectral_forward(ctx, spec_l, lidx, spec_r, ridx, (int)n, yaw, corr, ys, a2_in_yaw ? feats_r : nullptr,
                                   a2_in_yaw ? hs.sub_chunk(0, (int)n, false).a2raw : nullptr);
    if (rc) return rc;
  }
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t cn = (n - c0 < chunk) ? (n - c0) : chunk;
    if (corr_mode == 1) {
      OvnProfScope ps(ctx, OVN_K_CORR, stream);
      rc = ovn_corr_forward(lidx ? feats_l : feats_l + (size_t)c0 * feat_elems, lidx ? lidx + c0 : nullptr, feats_r,
                            ridx ? ridx + c0 : nullptr, (int)cn, fw, yaw + c0, corr ? corr + (size_t)c0 * fw : nullptr, stream,
                            ctx->corr_norm);
      if (rc) return rc;
    }
    int j = 0;
    for (int64_t q0 = 0; q0 < cn; q0 += sub, ++j) {
      const int64_t p0 = c0 + q0;
      const int np = (int)((cn - q0 < sub) ? (cn - q0) : sub);
      hipStream_t st = stream;
      if (nstreams == 2 && (j & 1)) {
        rc = fk.side(0, &st);
        if (rc) return rc;
      }
      const float* fl = lidx ? feats_l : feats_l + (size_t)p0 * feat_elems;
      const int32_t* li = lidx ? lidx + p0 : nullptr;
      const int32_t* ri = ridx ? ridx + p0 : nullptr;
      float* o2s = o2 + (size_t)q0 * o2_elems;
      const OvnDeltaSubScratch ds = hs.sub_chunk(j, np, ridx != nullptr);
      if (fused) {   // times its prepare kernels, the contraction kernel and c_conv2 separately
        unsigned* o2max = ds.o2max;
        float* part = o3 + (size_t)q0 * OVN_DENSE_PARTIALS;
        OvnSegPass sp{};
        if (seg) {
          sp = *seg;
          sp.pseg += p0;
          sp.state = hs.seg;
        }
        rc = ovn_delta_c12_f16x3_forward(ctx, fl, li, feats_r, ri, np, ds, o2s, st, (int)(p0 & 0x3fffffff),
                                          // a cache row belongs to a CANDIDATE: without an index list it moves with the feature pointer
                                          dcache_l ? (lidx ? dcache_l : dcache_l + (size_t)p0 * OVN_DELTA_CACHE_ELEMS) : nullptr, a2_in_yaw,
                                          seg ? &sp : nullptr);
        if (rc) return rc;
        if (p0 == 0) ctx->dbg_o2max = o2max;
        {   // c_conv3 + Flatten + Dense + sigmoid: one launch (the pair's last workgroup finishes it)
          OvnProfScope ps(ctx, OVN_K_C3, st);
          rc = ovn_c3_dense_forward(ctx, o2s, o2max, np, part, nullptr, ctx->c3_arrived + q0, overlap + p0, logit ? logit + p0 : nullptr, st);
        }
      } else {   // bf16x3: times its prepare kernels, the contraction kernel and c_conv2 separately
        float* o3s = o3 + (size_t)q0 * o3_elems;
        rc = ovn_delta_c12_bf16x3_forward(ctx, fl, li, feats_r, ri, np, ds, o2s, st, (int)(p0 & 0x3fffffff),
                                          a2_in_yaw);
        if (rc) return rc;
        int oh = 0, ow = 0;
        {
          OvnProfScope ps(ctx, OVN_K_C3, st);
          rc = ovn_conv_forward(ctx->head.c3, o2s, np, OVN_G, OVN_G, o3s, &oh, &ow, st);
        }
        if (rc) return rc;
        OvnProfScope ps(ctx, OVN_K_DENSE, st);
        rc = ovn_dense_sigmoid_forward(ctx, o3s, np, OVN_DENSE_IN, overlap + p0, logit ? logit + p0 : nullptr, st);
      }
      if (rc) return rc;
    }
  }
  return fk.join();
}

int ovn_heads(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
              int64_t n, float* overlap, int32_t* yaw, float* logit, float* corr, void* stream_) {
  OVN_REQUIRE(ctx && ctx->head_set, OVN_ERR_STATE, "ovn_heads: head weights not set");
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_heads: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_l && feats_r && overlap && yaw, OVN_ERR_ARG, "ovn_heads: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return delta_head_run(ctx, feats_l, lidx, feats_r, ridx, n, overlap, logit, yaw, corr, 1, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

int ovn_heads_spectral(ovn_ctx* ctx, const float* feats_l, const float* spec_l, const float* dcache_l, const int32_t* lidx,
                       const float* feats_r, const float* spec_r, const int32_t* ridx, int64_t n, float* overlap, int32_t* yaw,
                       float* logit, float* corr, void* stream_) {
  OVN_REQUIRE(ctx && ctx->head_set, OVN_ERR_STATE, "ovn_heads_spectral: head weights not set");
  OVN_REQUIRE(ctx_feat_w(ctx) == OVN_FEAT_W, OVN_ERR_ARG,
              "ovn_heads_spectral: the spectral correlation head needs 360-column feature volumes (the leg produces %d)", ctx_feat_w(ctx));
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_heads_spectral: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_l && feats_r && spec_l && spec_r && overlap && yaw, OVN_ERR_ARG, "ovn_heads_spectral: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return delta_head_run(ctx, feats_l, lidx, feats_r, ridx, n, overlap, logit, yaw, corr, 2, spec_l, spec_r,
                        ctx->head_mode == 1 ? dcache_l : nullptr, (hipStream_t)stream_);   // (rows serve the f16x3 mode only)
}

int ovn_delta_head(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx,
                   int64_t n, float* overlap, float* logit, void* stream_) {
  OVN_REQUIRE(ctx && ctx->head_set, OVN_ERR_STATE, "ovn_delta_head: head weights not set");
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_delta_head: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_l && feats_r && overlap, OVN_ERR_ARG, "ovn_delta_head: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return delta_head_run(ctx, feats_l, lidx, feats_r, ridx, n, overlap, logit, nullptr, nullptr, 0, nullptr, nullptr, nullptr, (hipStream_t)stream_);
}

int ovn_head_param_sizes(ovn_ctx* ctx, int64_t* sizes8) {
  OVN_REQUIRE(ctx && sizes8, OVN_ERR_ARG, "ovn_head_param_sizes: NULL argument");
  ovn_head_param_sizes_of(ctx->head_s, ctx_feat_w(ctx), sizes8);
  return OVN_OK;
}

int ovn_delta_head_grad(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int64_t n,
                        const float* target, int loss, float scale, float* grad, float* loss_dev, float* overlap, float* o2, float* o3,
                        void* stream_) {
  OVN_REQUIRE(ctx && feats_l && feats_r && target && grad && loss_dev, OVN_ERR_ARG, "ovn_delta_head_grad: NULL argument");
  OVN_REQUIRE(n >= 1 && n < (1ll << 31), OVN_ERR_ARG, "ovn_delta_head_grad: bad n %lld", (long long)n);
  OVN_REQUIRE(loss == 0 || loss == 1, OVN_ERR_ARG, "ovn_delta_head_grad: loss %d (0 = sigmoid loss, 1 = squared error)", loss);
  OVN_REQUIRE(isfinite(scale), OVN_ERR_ARG, "ovn_delta_head_grad: scale is not finite");
  OVN_REQUIRE(ctx->head_set, OVN_ERR_STATE, "ovn_delta_head_grad: head weights not set");
  OVN_ON_DEVICE(ctx->device);
  return ovn_delta_head_grad_run(ctx, ctx_feat_w(ctx), feats_l, lidx, feats_r, ridx, n, target, loss, scale, grad, loss_dev, overlap, o2,
                                 o3, (hipStream_t)stream_);
}

int ovn_heads_feature_grad(ovn_ctx* ctx, const float* feats_l, const int32_t* lidx, const float* feats_r, const int32_t* ridx, int64_t n,
                           const float* target, const int32_t* yaw_bin, int loss, float overlap_scale, float yaw_scale,
                           float min_overlap_for_angle, float* dfeat_l, float* dfeat_r, float* head_grad, float* loss_dev, float* overlap,
                           float* corr, void* stream_) {
  OVN_REQUIRE(ctx && feats_l && feats_r && target && dfeat_l && dfeat_r && loss_dev, OVN_ERR_ARG, "ovn_heads_feature_grad: NULL argument");
  OVN_REQUIRE(n >= 1 && n < (1ll << 31), OVN_ERR_ARG, "ovn_heads_feature_grad: bad n %lld", (long long)n);
  OVN_REQUIRE(loss == 0 || loss == 1, OVN_ERR_ARG, "ovn_heads_feature_grad: loss %d (0 = sigmoid loss, 1 = squared error)", loss);
  OVN_REQUIRE(isfinite(overlap_scale) && isfinite(yaw_scale) && isfinite(min_overlap_for_angle), OVN_ERR_ARG,
              "ovn_heads_feature_grad: a scale or the threshold is not finite");
  OVN_REQUIRE(ctx->head_set, OVN_ERR_STATE, "ovn_heads_feature_grad: head weights not set");
  const bool yaw_on = yaw_bin != nullptr && yaw_scale != 0.f;
  OVN_REQUIRE(!yaw_on || ctx->corr_norm == 0, OVN_ERR_STATE,
              "ovn_heads_feature_grad: the yaw loss is differentiated for correlation normalisation 'none' only (mode %d is set)",
              ctx->corr_norm);
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const int fw = ctx_feat_w(ctx);
  const size_t bytes = (size_t)n * fw * OVN_FEAT_C * sizeof(float);
  OVN_HIP_CHECK(hipMemsetAsync(dfeat_l, 0, bytes, stream));
  OVN_HIP_CHECK(hipMemsetAsync(dfeat_r, 0, bytes, stream));
  OVN_HIP_CHECK(hipMemsetAsync(loss_dev, 0, 2 * sizeof(float), stream));
  int rc = OVN_OK;
  if (overlap_scale != 0.f) {
    rc = ovn_delta_head_grad_run(ctx, fw, feats_l, lidx, feats_r, ridx, n, target, loss, overlap_scale, head_grad, loss_dev, overlap, nullptr,
                                 nullptr, stream, dfeat_l, dfeat_r);
  } else {
    if (head_grad) {
      int64_t sz[8], total = 0;
      ovn_head_param_sizes_of(ctx->head_s, fw, sz);
      for (int t = 0; t < 8; ++t) total += sz[t];
      OVN_HIP_CHECK(hipMemsetAsync(head_grad, 0, (size_t)total * sizeof(float), stream));
    }
    if (overlap)
      rc = ovn_delta_head_grad_run(ctx, fw, feats_l, lidx, feats_r, ridx, n, target, loss, 0.f, nullptr, nullptr, overlap, nullptr, nullptr,
                                   stream, nullptr, nullptr, true);
  }
  if (rc) return rc;
  if (yaw_on || corr)
    rc = ovn_yaw_grad_run(ctx, fw, feats_l, lidx, feats_r, ridx, n, target, yaw_on ? yaw_bin : nullptr, yaw_scale, min_overlap_for_angle,
                          dfeat_l, dfeat_r, loss_dev + 1, corr, stream);
  return rc;
}

int ovn_delta_cache(ovn_ctx* ctx, const float* feats_dev, int64_t n, float* cache_dev, void* stream) {
  OVN_REQUIRE(ctx && ctx->head_set, OVN_ERR_STATE, "ovn_delta_cache: head weights not set");
  OVN_REQUIRE(ctx_feat_w(ctx) == OVN_FEAT_W, OVN_ERR_ARG,
              "ovn_delta_cache: Delta cache rows exist for 360-column feature volumes only (the leg produces %d)", ctx_feat_w(ctx));
  OVN_REQUIRE(n >= 0 && n < (1ll << 24), OVN_ERR_ARG, "ovn_delta_cache: bad n");
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_dev && cache_dev, OVN_ERR_ARG, "ovn_delta_cache: NULL buffer");
  OVN_REQUIRE((reinterpret_cast<uintptr_t>(cache_dev) & 15) == 0, OVN_ERR_ARG, "ovn_delta_cache: cache_dev must be 16-byte aligned");
  OVN_REQUIRE(ctx->head_s == OVN_S, OVN_ERR_STATE, "ovn_delta_cache: only the default head geometry (conv1size 15) has a Delta cache");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_DELTA_PREP, (hipStream_t)stream);
  return ovn_delta_cache_forward(ctx, feats_dev, (int)n, cache_dev, (hipStream_t)stream);
}

int ovn_set_head_geometry(ovn_ctx* ctx, int conv1size) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_head_geometry: ctx is NULL");
  OVN_REQUIRE(!ctx->head_set, OVN_ERR_STATE, "ovn_set_head_geometry: call it before ovn_set_head_weights");
  const int fw = ctx_feat_w(ctx);
  OVN_REQUIRE(conv1size >= 1 && fw / conv1size >= 3, OVN_ERR_ARG,
              "ovn_set_head_geometry: conv1size %d leaves fewer than 3 x 3 groups of the %d columns for c_conv3", conv1size, fw);
  ctx->head_s = conv1size;
  ctx->head_g = fw / conv1size;
  return OVN_OK;
}

int ovn_set_head_pipeline(ovn_ctx* ctx, int64_t chunk_pairs, int64_t sub_chunk_pairs, int streams, int yaw_on_side_stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_head_pipeline: ctx is NULL");
  OVN_REQUIRE(chunk_pairs >= 1 && chunk_pairs <= (1 << 20), OVN_ERR_ARG, "ovn_set_head_pipeline: chunk_pairs %lld", (long long)chunk_pairs);
  OVN_REQUIRE(sub_chunk_pairs >= 0, OVN_ERR_ARG, "ovn_set_head_pipeline: sub_chunk_pairs %lld", (long long)sub_chunk_pairs);
  OVN_REQUIRE(streams == 1 || streams == 2, OVN_ERR_ARG, "ovn_set_head_pipeline: streams %d (1 or 2)", streams);
  ctx->head_chunk = chunk_pairs;
  ctx->head_sub = sub_chunk_pairs;
  ctx->head_streams = streams;
  ctx->head_yaw_side = yaw_on_side_stream ? 1 : 0;
  return OVN_OK;
}

int ovn_get_head_pipeline(ovn_ctx* ctx, int64_t* chunk_pairs, int64_t* sub_chunk_pairs, int* streams, int* yaw_on_side_stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_get_head_pipeline: ctx is NULL");
  if (chunk_pairs) *chunk_pairs = ctx->head_chunk;
  if (sub_chunk_pairs) *sub_chunk_pairs = ctx->head_sub;
  if (streams) *streams = ctx->head_streams;
  if (yaw_on_side_stream) *yaw_on_side_stream = ctx->head_yaw_side;
  return OVN_OK;
}

int ovn_best_match(ovn_ctx* ctx, const float* overlap, const int32_t* yaw, const int32_t* ids, int64_t n, float threshold,
                   int64_t index_offset, int32_t* out, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_best_match: ctx is NULL");
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_best_match: bad n");
  OVN_REQUIRE(index_offset >= 0 && index_offset + n < (1ll << 31), OVN_ERR_ARG, "ovn_best_match: bad index_offset");
  OVN_REQUIRE(out != nullptr && (n == 0 || overlap != nullptr), OVN_ERR_ARG, "ovn_best_match: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return ovn_best_match_forward(overlap, yaw, ids, (int)n, threshold, (int)index_offset, out, (hipStream_t)stream);
}

int ovn_top_k(ovn_ctx* ctx, const float* overlap, const int32_t* yaw, const int32_t* ids, int64_t n, int k, float threshold,
              int64_t index_offset, int32_t* out, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_top_k: ctx is NULL");
  OVN_REQUIRE(k >= 1 && k <= OVN_TOP_K_MAX, OVN_ERR_ARG, "ovn_top_k: k must be in 1..OVN_TOP_K_MAX (1024)");
  OVN_REQUIRE(n >= 0 && n < (1ll << 31), OVN_ERR_ARG, "ovn_top_k: bad n");
  OVN_REQUIRE(index_offset >= 0 && index_offset + n < (1ll << 31), OVN_ERR_ARG, "ovn_top_k: bad index_offset");
  OVN_REQUIRE(out != nullptr && (n == 0 || overlap != nullptr), OVN_ERR_ARG, "ovn_top_k: NULL buffer");
  OVN_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, OVN_ERR_ARG, "ovn_top_k: out_dev is not 16-byte aligned");
  OVN_ON_DEVICE(ctx->device);
  return ovn_top_k_forward(overlap, yaw, ids, (int)n, k, threshold, (int)index_offset, out, (hipStream_t)stream);
}

int ovn_icp_register(ovn_ctx* ctx, const float* vertex, const float* normal, const float* range, int n_scans, int proj_h, int proj_w,
                     double fov_up_deg, double fov_down_deg, double max_range, const int32_t* src_idx, const int32_t* tgt_idx,
                     int64_t n_pairs, const double* init_pose, int iterations, double max_dist, double cos_min, double huber,
                     int min_inliers, double* pose, double* stats, double* system, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_icp_register: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0 && proj_h > 0 && proj_w > 0 && n_pairs >= 0 && n_pairs < (1ll << 31), OVN_ERR_ARG,
              "ovn_icp_register: bad sizes");
  OVN_REQUIRE((int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG, "ovn_icp_register: H*W exceeds 2^31 - 1");
  OVN_REQUIRE(iterations >= 0 && iterations <= 1000, OVN_ERR_ARG, "ovn_icp_register: iterations must be in 0..1000");
  OVN_REQUIRE(max_dist > 0.0 && cos_min > 0.0 && huber > 0.0 && max_range > 0.0, OVN_ERR_ARG,
              "ovn_icp_register: max_dist, cos_min, huber and max_range must be > 0");
  OVN_REQUIRE(max_dist < 1e18 && cos_min <= 1.0 && huber < 1e18, OVN_ERR_ARG, "ovn_icp_register: gate out of range");
  OVN_REQUIRE(min_inliers >= 0, OVN_ERR_ARG, "ovn_icp_register: min_inliers < 0");
  OVN_REQUIRE(fabs(fov_up_deg) + fabs(fov_down_deg) > 0.0, OVN_ERR_ARG, "ovn_icp_register: empty vertical field of view");
  if (n_pairs == 0) return OVN_OK;
  OVN_REQUIRE(src_idx && tgt_idx && init_pose && pose && stats, OVN_ERR_ARG, "ovn_icp_register: NULL buffer");
  OVN_REQUIRE(n_scans == 0 || (vertex && normal && range), OVN_ERR_ARG, "ovn_icp_register: NULL image buffer");
  OVN_ON_DEVICE(ctx->device);
  return ovn_icp_register_forward(vertex, normal, range, n_scans, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, src_idx,
                                  tgt_idx, (int)n_pairs, init_pose, iterations, max_dist, cos_min, huber, min_inliers, pose, stats,
                                  system, (hipStream_t)stream);
}

// ---- Monte Carlo localization (mcl.hip) ------------------------------------------------------------------------------------------
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int ovn_mcl_predict(ovn_ctx* ctx, float* particles, int n_particles, double dx, double dy, double dtheta, double sigma_x, double sigma_y,
                    double sigma_theta, uint64_t seed, uint64_t step, const int32_t* cell_frame, double origin_x, double origin_y,
                    double resolution, int nx, int ny, int n_frames, int32_t* particle_frame, int32_t* frame_slot, int32_t* frame_list,
                    int32_t* record, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_mcl_predict: ctx is NULL");
  OVN_REQUIRE(n_particles >= 1 && n_particles <= OVN_MCL_MAX_PARTICLES, OVN_ERR_ARG,
              "ovn_mcl_predict: n_particles %d outside 1..%d", n_particles, OVN_MCL_MAX_PARTICLES);
  OVN_REQUIRE(nx >= 1 && ny >= 1 && (int64_t)nx * ny <= 2147483647ll, OVN_ERR_ARG, "ovn_mcl_predict: grid %d x %d outside 1..2^31 - 1 cells",
              nx, ny);
  OVN_REQUIRE(n_frames >= 1, OVN_ERR_ARG, "ovn_mcl_predict: n_frames %d < 1", n_frames);
  OVN_REQUIRE(resolution > 0.0 && resolution < INFINITY, OVN_ERR_ARG, "ovn_mcl_predict: resolution must be > 0");
  OVN_REQUIRE(particles && cell_frame && particle_frame && frame_slot && frame_list && record, OVN_ERR_ARG,
              "ovn_mcl_predict: NULL buffer");
  OVN_REQUIRE(aligned16(particles), OVN_ERR_ARG, "ovn_mcl_predict: particles_dev is not 16-byte aligned");
  OVN_REQUIRE(aligned16(record), OVN_ERR_ARG, "ovn_mcl_predict: record_dev is not 16-byte aligned");
  OVN_ON_DEVICE(ctx->device);
  const double motion6[6] = {dx, dy, dtheta, sigma_x, sigma_y, sigma_theta};
  return ovn_mcl_predict_forward(particles, n_particles, motion6, seed, step, cell_frame, origin_x, origin_y, resolution, nx, ny,
                                 n_frames, particle_frame, frame_slot, frame_list, record, (hipStream_t)stream);
}

int ovn_mcl_update(ovn_ctx* ctx, float* particles, int n_particles, const int32_t* particle_frame, const int32_t* frame_slot,
                   const float* frame_yaw, int n_frames, const float* overlap, const int32_t* yaw, int n_scores, double sigma_yaw_deg,
                   double eps_yaw, double overlap_min, double* estimate, double* spread, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_mcl_update: ctx is NULL");
  OVN_REQUIRE(n_particles >= 1 && n_particles <= OVN_MCL_MAX_PARTICLES, OVN_ERR_ARG,
              "ovn_mcl_update: n_particles %d outside 1..%d", n_particles, OVN_MCL_MAX_PARTICLES);
  OVN_REQUIRE(n_frames >= 1, OVN_ERR_ARG, "ovn_mcl_update: n_frames %d < 1", n_frames);
  OVN_REQUIRE(n_scores >= 0 && n_scores <= n_frames, OVN_ERR_ARG, "ovn_mcl_update: n_scores %d outside [0, n_frames]", n_scores);
  OVN_REQUIRE(sigma_yaw_deg > 0.0 && sigma_yaw_deg < INFINITY, OVN_ERR_ARG, "ovn_mcl_update: sigma_yaw_deg must be > 0");
  OVN_REQUIRE(overlap_min > 0.0 && overlap_min < INFINITY, OVN_ERR_ARG, "ovn_mcl_update: overlap_min must be > 0");
  OVN_REQUIRE(eps_yaw >= 0.0 && eps_yaw <= 1.0, OVN_ERR_ARG, "ovn_mcl_update: eps_yaw outside [0, 1]");
  OVN_REQUIRE(particles && particle_frame && frame_slot && frame_yaw && estimate, OVN_ERR_ARG, "ovn_mcl_update: NULL buffer");
  OVN_REQUIRE(n_scores == 0 || (overlap && yaw), OVN_ERR_ARG, "ovn_mcl_update: NULL score buffer with n_scores %d", n_scores);
  OVN_REQUIRE(aligned16(particles), OVN_ERR_ARG, "ovn_mcl_update: particles_dev is not 16-byte aligned");
  OVN_REQUIRE(aligned16(estimate), OVN_ERR_ARG, "ovn_mcl_update: estimate_dev is not 16-byte aligned");
  OVN_ON_DEVICE(ctx->device);
  return ovn_mcl_update_forward(particles, n_particles, particle_frame, frame_slot, frame_yaw, n_frames, overlap, yaw, n_scores,
                                sigma_yaw_deg, eps_yaw, overlap_min, estimate, spread, (hipStream_t)stream);
}

int ovn_mcl_resample(ovn_ctx* ctx, const float* particles, int n_particles, uint64_t seed, uint64_t step, float* out_particles,
                     int n_out, int32_t* ancestor, int32_t* record, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_mcl_resample: ctx is NULL");
  OVN_REQUIRE(n_particles >= 1 && n_particles <= OVN_MCL_MAX_PARTICLES, OVN_ERR_ARG,
              "ovn_mcl_resample: n_particles %d outside 1..%d", n_particles, OVN_MCL_MAX_PARTICLES);
  OVN_REQUIRE(n_out >= 1 && n_out <= OVN_MCL_MAX_PARTICLES, OVN_ERR_ARG, "ovn_mcl_resample: n_out %d outside 1..%d", n_out,
              OVN_MCL_MAX_PARTICLES);
  OVN_REQUIRE(particles && out_particles && ancestor && record, OVN_ERR_ARG, "ovn_mcl_resample: NULL buffer");
  OVN_REQUIRE(aligned16(particles) && aligned16(out_particles), OVN_ERR_ARG, "ovn_mcl_resample: particle buffers must be 16-byte aligned");
  OVN_REQUIRE(aligned16(record), OVN_ERR_ARG, "ovn_mcl_resample: record_dev is not 16-byte aligned");
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(particles), b = reinterpret_cast<uintptr_t>(out_particles);
    OVN_REQUIRE(a + 16ull * n_particles <= b || b + 16ull * n_out <= a, OVN_ERR_ARG,
                "ovn_mcl_resample: out_particles_dev overlaps particles_dev");
  }
  OVN_ON_DEVICE(ctx->device);
  return ovn_mcl_resample_forward(particles, n_particles, seed, step, out_particles, n_out, ancestor, record, (hipStream_t)stream);
}

// ---- segmented batches ---------------------------------------------------------------------------------------------------------
// The host segment table (offsets, and the query of every segment when it is given) is validated, staged in a context-owned pinned
// buffer and copied to seg_dev on `stream`; device space for the per-pair right index and segment index follows it.  The pinned buffer
// is rewritten only after the previous call's copy has left it (seg_ev).
struct SegTable {   // ONE layout for the pinned mirror and for seg_dev: offsets (B + 1) | query_idx (B) | ridx (n) | pseg (n), each optional but the first
  int64_t* offs = nullptr;
  int32_t *qidx = nullptr, *ridx = nullptr, *pseg = nullptr;
  SegTable() = default;
  SegTable(OvnCarver& c, int64_t B, bool with_qidx, int64_t n_ridx, int64_t n_pseg) {
    offs = c.take<int64_t>((size_t)B + 1);
    qidx = with_qidx ? c.take<int32_t>((size_t)B) : nullptr;
    ridx = n_ridx ? c.take<int32_t>((size_t)n_ridx) : nullptr;
    pseg = n_pseg ? c.take<int32_t>((size_t)n_pseg) : nullptr;
  }
};
static const char* seg_offsets_error(const int64_t* offs, int64_t B, int64_t* n_out) {
  if (B < 0 || B >= (1ll << 31)) return "B outside [0, 2^31)";
  if (!offs) return "seg_offsets is NULL";
  if (offs[0] != 0) return "seg_offsets[0] != 0";
  for (int64_t b = 0; b < B; ++b)
    if (offs[b + 1] < offs[b]) return "seg_offsets decrease";
  if (offs[B] >= (1ll << 31)) return "more than 2^31 - 1 pairs";
  *n_out = offs[B];
  return nullptr;
}

static int seg_stage(ovn_ctx* ctx, const int64_t* offs, const int32_t* qidx, int64_t B, int64_t n_ridx, int64_t n_pseg,
                     hipStream_t stream, SegTable* dev) {
  const size_t staged = ovn_scratch_bytes<SegTable>(B, qidx != nullptr, (int64_t)0, (int64_t)0);   // what the host fills in
  const size_t need = ovn_scratch_bytes<SegTable>(B, qidx != nullptr, n_ridx, n_pseg);
  if (!ctx->seg_ev) {
    OVN_HIP_CHECK(hipEventCreateWithFlags(&ctx->seg_ev, hipEventDisableTiming));
    OVN_HIP_CHECK(hipEventCreateWithFlags(&ctx->seg_done, hipEventDisableTiming));
  }
  if (ctx->seg_ev_pending) {
    OVN_HIP_CHECK(hipEventSynchronize(ctx->seg_ev));              // the previous table has left the pinned buffer
    OVN_HIP_CHECK(hipStreamWaitEvent(stream, ctx->seg_done, 0));  // and its kernels are done with seg_dev, whatever their stream
    ctx->seg_ev_pending = false;
  }
  if (need > ctx->seg_cap) {
    OVN_HIP_CHECK(hipStreamSynchronize(stream));       // earlier launches may still read the old device table
    if (ctx->seg_dev) (void)hipFree(ctx->seg_dev);
    if (ctx->seg_host) (void)hipHostFree(ctx->seg_host);
    ctx->seg_dev = ctx->seg_host = nullptr;
    ctx->seg_cap = 0;
    const size_t want = need + need / 2;
    OVN_HIP_CHECK(hipMalloc(&ctx->seg_dev, want));
    OVN_HIP_CHECK(hipHostMalloc(&ctx->seg_host, want, hipHostMallocDefault));
    ctx->seg_cap = want;
  }
  OvnCarver hc(ctx->seg_host), dc(ctx->seg_dev);
  const SegTable h(hc, B, qidx != nullptr, n_ridx, n_pseg);
  *dev = SegTable(dc, B, qidx != nullptr, n_ridx, n_pseg);
  memcpy(h.offs, offs, (size_t)(B + 1) * sizeof(int64_t));
  if (qidx) memcpy(h.qidx, qidx, (size_t)B * sizeof(int32_t));
  OVN_HIP_CHECK(hipMemcpyAsync(ctx->seg_dev, ctx->seg_host, staged, hipMemcpyHostToDevice, stream));
  OVN_HIP_CHECK(hipEventRecord(ctx->seg_ev, stream));
  ctx->seg_ev_pending = true;
  return OVN_OK;
}

// the last kernel of a segmented call that reads seg_dev has been enqueued on `stream`
static int seg_release(ovn_ctx* ctx, hipStream_t stream) {
  OVN_HIP_CHECK(hipEventRecord(ctx->seg_done, stream));
  return OVN_OK;
}

static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int ovn_heads_segments(ovn_ctx* ctx, const float* feats_pool, const float* spec_pool, const float* dcache_pool,
                       const int32_t* cand_idx, const float* feats_q, const float* spec_q, const int32_t* query_idx,
                       const int64_t* seg_offsets, int64_t B, int64_t n, float* overlap, int32_t* yaw, float* logit, float* corr,
                       void* stream_) {
  OVN_REQUIRE(ctx && ctx->head_set, OVN_ERR_STATE, "ovn_heads_segments: head weights not set");
  int64_t total = 0;
  const char* bad = seg_offsets_error(seg_offsets, B, &total);
  OVN_REQUIRE(bad == nullptr, OVN_ERR_ARG, "ovn_heads_segments: %s", bad);
  OVN_REQUIRE(n == total, OVN_ERR_ARG, "ovn_heads_segments: n = %lld but seg_offsets[B] = %lld", (long long)n, (long long)total);
  OVN_REQUIRE(B == 0 || query_idx != nullptr, OVN_ERR_ARG, "ovn_heads_segments: query_idx is NULL");
  for (int64_t b = 0; b < B; ++b)
    OVN_REQUIRE(query_idx[b] >= 0, OVN_ERR_ARG, "ovn_heads_segments: query_idx[%lld] = %d < 0", (long long)b, query_idx[b]);
  if (n == 0) return OVN_OK;
  OVN_REQUIRE(feats_pool && feats_q && cand_idx && overlap && yaw, OVN_ERR_ARG, "ovn_heads_segments: NULL buffer");
  OVN_REQUIRE((spec_pool == nullptr) == (spec_q == nullptr), OVN_ERR_ARG, "ovn_heads_segments: spec_pool and spec_q go together");
  const int fw = ctx_feat_w(ctx);
  OVN_REQUIRE(spec_pool == nullptr || fw == OVN_FEAT_W, OVN_ERR_ARG,
              "ovn_heads_segments: the spectral correlation head needs 360-column feature volumes (the leg produces %d)", fw);
  OVN_REQUIRE(!misaligned(feats_pool, 4) && !misaligned(feats_q, 4) && !misaligned(cand_idx, 4) && !misaligned(overlap, 4) &&
                  !misaligned(yaw, 4) && !misaligned(logit, 4) && !misaligned(corr, 4) && !misaligned(spec_pool, 4) &&
                  !misaligned(spec_q, 4) && !misaligned(dcache_pool, 16),
              OVN_ERR_ARG, "ovn_heads_segments: misaligned buffer (4 bytes; dcache_pool 16 bytes)");
  OVN_ON_DEVICE(ctx->device);
  hipStream_t stream = (hipStream_t)stream_;
  const bool spectral = spec_pool != nullptr;
  const int corr_mode = spectral ? 2 : 1;
  // f16x3 at W = 360 with conv1size 15 and compaction on: segmented passes (each segment's query state once, its compacted K walk and
  // the Delta cache rows, as in its 1-vs-N sweep).  Every other mode and geometry -- and f16x3 with compaction off, whose 1-vs-N walk
  // is the 128-channel walk of an indexed pair -- is the same per pair in the indexed form: one indexed pass over all pairs.
  const bool segmented = ctx->head_mode == 1 && fw == OVN_FEAT_W && ctx->head_s == OVN_S && ctx->head_compact;
  SegTable tab;
  int rc = seg_stage(ctx, seg_offsets, query_idx, B, n, segmented ? n : 0, stream, &tab);
  if (rc) return rc;
  int64_t* offs_dev = tab.offs;
  int32_t *qidx_dev = tab.qidx, *ridx = tab.ridx, *pseg = tab.pseg;
  {
    OvnProfScope ps(ctx, OVN_K_DELTA_PREP, stream);
    rc = ovn_segment_ridx_forward(offs_dev, qidx_dev, (int)B, (int)n, ridx, pseg, stream);
    if (rc) return rc;
  }
  if (!segmented) {
    rc = delta_head_run(ctx, feats_pool, cand_idx, feats_q, ridx, n, overlap, logit, yaw, corr, corr_mode, spec_pool, spec_q, nullptr, stream);
    return rc ? rc : seg_release(ctx, stream);
  }
  // passes of at most head_chunk pairs and OVN_SEG_PASS_MAX segments (a segment may straddle two passes: its state is computed in both)
  const float* dc = spectral ? dcache_pool : nullptr;   // (rows serve ovn_heads_spectral's sweeps)
  const int64_t* o = seg_offsets;
  auto seg_of = [&](int64_t p) { return (int64_t)(std::upper_bound(o, o + B + 1, p) - o) - 1; };   // the segment holding pair p
  for (int64_t p0 = 0; p0 < n;) {
    const int64_t b0 = seg_of(p0);
    int64_t p1 = std::min(n, p0 + ctx->head_chunk);
    if (seg_of(p1 - 1) - b0 + 1 > OVN_SEG_PASS_MAX) p1 = o[b0 + OVN_SEG_PASS_MAX];
    const int64_t np = p1 - p0;
    OvnSegPass sp{pseg + p0, qidx_dev, offs_dev, (int)b0, (int)(seg_of(p1 - 1) - b0 + 1), {}};
    rc = delta_head_run(ctx, feats_pool, cand_idx + p0, feats_q, ridx + p0, np, overlap + p0, logit ? logit + p0 : nullptr, yaw + p0,
                        corr ? corr + (size_t)p0 * fw : nullptr, corr_mode, spec_pool, spec_q, dc, stream, &sp);
    if (rc) return rc;
    p0 = p1;
  }
  return seg_release(ctx, stream);
}

int ovn_top_k_segments(ovn_ctx* ctx, const float* overlap, const int32_t* yaw, const int32_t* ids, const int64_t* seg_offsets,
                       int64_t B, int k, float threshold, int32_t* out, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_top_k_segments: ctx is NULL");
  OVN_REQUIRE(k >= 1 && k <= OVN_TOP_K_MAX, OVN_ERR_ARG, "ovn_top_k_segments: k must be in 1..OVN_TOP_K_MAX (1024)");
  int64_t n = 0;
  const char* bad = seg_offsets_error(seg_offsets, B, &n);
  OVN_REQUIRE(bad == nullptr, OVN_ERR_ARG, "ovn_top_k_segments: %s", bad);
  if (B == 0) return OVN_OK;
  OVN_REQUIRE(out != nullptr && (n == 0 || overlap != nullptr), OVN_ERR_ARG, "ovn_top_k_segments: NULL buffer");
  OVN_REQUIRE(!misaligned(out, 16), OVN_ERR_ARG, "ovn_top_k_segments: out_dev is not 16-byte aligned");
  OVN_REQUIRE(!misaligned(overlap, 4) && !misaligned(yaw, 4) && !misaligned(ids, 4), OVN_ERR_ARG,
              "ovn_top_k_segments: misaligned buffer");
  OVN_ON_DEVICE(ctx->device);
  SegTable tab;
  int rc = seg_stage(ctx, seg_offsets, nullptr, B, 0, 0, (hipStream_t)stream, &tab);
  if (rc) return rc;
  rc = ovn_top_k_segments_forward(overlap, yaw, ids, tab.offs, (int)B, k, threshold, out, (hipStream_t)stream);
  return rc ? rc : seg_release(ctx, (hipStream_t)stream);
}

int ovn_project(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                int64_t max_points_per_scan, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                double max_range, float* range_dev, float* vertex_dev, float* intensity_dev, int32_t* idx_dev,
                float* normal_dev, float* stacked_dev, int use_depth, int use_normals, int use_intensity, void* stream) {
  // the kernels form H * W and a pixel's index in 32 bits, and the scatter's grid carries the scan in its y dimension
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_project: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(n_scans <= 65535, OVN_ERR_ARG, "ovn_project: %d scans, at most 65535 per call", n_scans);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_project: ctx is NULL");
  OVN_REQUIRE(n_scans == 0 || (points_dev || max_points_per_scan == 0), OVN_ERR_ARG, "ovn_project: points is NULL");
  OVN_REQUIRE(n_scans == 0 || offsets_dev, OVN_ERR_ARG, "ovn_project: offsets is NULL");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_PROJ, (hipStream_t)stream);
  return ovn_project_forward(ctx, points_dev, offsets_dev, n_scans, max_points_per_scan, proj_h, proj_w, fov_up_deg,
                             fov_down_deg, max_range, range_dev, vertex_dev, intensity_dev, idx_dev, normal_dev,
                             stacked_dev, use_depth, use_normals, use_intensity, (hipStream_t)stream);
}

int ovn_project_semantic(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                         int64_t max_points_per_scan, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                         double max_range, const float* probs_dev, int n_classes, float* range_dev, float* vertex_dev,
                         float* intensity_dev, int32_t* idx_dev, float* normal_dev, float* semantic_dev, int32_t* sem_idx_dev,
                         float* stacked_dev, int use_depth, int use_normals, int use_semantic, int use_intensity, void* stream) {
  OVN_REQUIRE(n_classes >= 1 && n_classes <= OVN_SEMANTIC_CLASSES_MAX, OVN_ERR_ARG,
              "ovn_project_semantic: n_classes %d outside 1..%d", n_classes, OVN_SEMANTIC_CLASSES_MAX);
  OVN_REQUIRE(probs_dev || !(semantic_dev || (stacked_dev && use_semantic)), OVN_ERR_ARG,
              "ovn_project_semantic: probabilities requested but probs is NULL");
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_project_semantic: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_project_semantic: ctx is NULL");
  OVN_REQUIRE(n_scans == 0 || (points_dev || max_points_per_scan == 0), OVN_ERR_ARG, "ovn_project_semantic: points is NULL");
  OVN_REQUIRE(n_scans == 0 || offsets_dev, OVN_ERR_ARG, "ovn_project_semantic: offsets is NULL");
  OVN_ON_DEVICE(ctx->device);
  OvnProfScope ps(ctx, OVN_K_PROJ, (hipStream_t)stream);
  return ovn_project_semantic_forward(ctx, points_dev, offsets_dev, n_scans, max_points_per_scan, proj_h, proj_w, fov_up_deg,
                                      fov_down_deg, max_range, probs_dev, n_classes, range_dev, vertex_dev, intensity_dev, idx_dev,
                                      normal_dev, semantic_dev, sem_idx_dev, stacked_dev, use_depth, use_normals, use_semantic,
                                      use_intensity, (hipStream_t)stream);
}

int ovn_projection_angles(ovn_ctx* ctx, const float* points_dev, int64_t n_points, int proj_h, int proj_w, double fov_up_deg,
                          double fov_down_deg, double max_range, float* yaw_dev, float* pitch_dev, int32_t* pixel_dev,
                          void* stream) {
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_projection_angles: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_projection_angles: ctx is NULL");
  OVN_REQUIRE(n_points >= 0 && proj_h > 0 && proj_w > 0, OVN_ERR_ARG, "ovn_projection_angles: bad sizes");
  if (n_points == 0) return OVN_OK;
  OVN_REQUIRE(points_dev != nullptr, OVN_ERR_ARG, "ovn_projection_angles: points is NULL");
  OVN_ON_DEVICE(ctx->device);
  return ovn_projection_angles_forward(points_dev, n_points, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, yaw_dev,
                                       pitch_dev, pixel_dev, (hipStream_t)stream, ctx->proj_trig);
}

int ovn_normals(ovn_ctx* ctx, const float* range_dev, const float* vertex_dev, int n_scans, int proj_h, int proj_w,
                float* normal_dev, void* stream) {
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_normals: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_normals: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0 && proj_h > 0 && proj_w > 0, OVN_ERR_ARG, "ovn_normals: bad sizes");
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(range_dev && vertex_dev && normal_dev, OVN_ERR_ARG, "ovn_normals: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return ovn_normals_forward(range_dev, vertex_dev, n_scans, proj_h, proj_w, normal_dev, (hipStream_t)stream);
}

int ovn_render_scans(ovn_ctx* ctx, const float* vertices_dev, int64_t n_vertices, const int32_t* triangles_dev, int64_t n_triangles,
                     const float* bvh_nodes_dev, const int32_t* bvh_order_dev, int64_t bvh_leaves, const double* poses_dev,
                     int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev, const float* sin_az_dev,
                     const float* cos_pitch_dev, const float* sin_pitch_dev, double max_range, float* range_dev, int32_t* tri_id_dev,
                     float* vertex_dev, float* normal_dev, float* stacked_dev, int use_depth, int use_normals, int use_intensity,
                     int use_semantic, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_render_scans: ctx is NULL");
  OVN_REQUIRE(n_vertices >= 1 && n_vertices <= 2147483647ll, OVN_ERR_ARG, "ovn_render_scans: %lld vertices outside 1 .. 2^31 - 1",
              (long long)n_vertices);
  OVN_REQUIRE(n_triangles >= 1 && n_triangles <= OVN_RENDER_MAX_TRIANGLES, OVN_ERR_ARG,
              "ovn_render_scans: %lld triangles outside 1 .. 2^27", (long long)n_triangles);
  OVN_REQUIRE(n_scans >= 0 && n_scans <= 2147483647ll, OVN_ERR_ARG, "ovn_render_scans: bad n_scans %lld", (long long)n_scans);
  OVN_REQUIRE(proj_h >= 1 && proj_w >= 1 && (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_render_scans: image %d x %d outside 1 .. 2^31 - 1 pixels", proj_h, proj_w);
  OVN_REQUIRE(max_range > 0.0, OVN_ERR_ARG, "ovn_render_scans: max_range must be > 0");
  OVN_REQUIRE(!use_intensity && !use_semantic, OVN_ERR_ARG,
              "ovn_render_scans: a rendered scan has no intensity and no class probabilities (use_intensity %d, use_semantic %d)",
              use_intensity, use_semantic);
  OVN_REQUIRE(vertices_dev && triangles_dev, OVN_ERR_ARG, "ovn_render_scans: NULL mesh buffer");
  OVN_REQUIRE((bvh_nodes_dev != nullptr) == (bvh_order_dev != nullptr), OVN_ERR_ARG,
              "ovn_render_scans: the hierarchy is both arrays or neither");
  if (bvh_nodes_dev) {
    OVN_REQUIRE(bvh_leaves >= 1 && bvh_leaves <= OVN_RENDER_MAX_TRIANGLES / OVN_RENDER_LEAF_TRIANGLES &&
                    (bvh_leaves & (bvh_leaves - 1)) == 0 && bvh_leaves * OVN_RENDER_LEAF_TRIANGLES >= n_triangles,
                OVN_ERR_ARG, "ovn_render_scans: %lld leaves: not a power of two in 1 .. 2^25 that holds %lld triangles",
                (long long)bvh_leaves, (long long)n_triangles);
    OVN_REQUIRE(aligned16(bvh_nodes_dev), OVN_ERR_ARG, "ovn_render_scans: bvh_nodes_dev is not 16-byte aligned");
  }
  OVN_REQUIRE(!vertex_dev || aligned16(vertex_dev), OVN_ERR_ARG, "ovn_render_scans: vertex_dev is not 16-byte aligned");
  use_depth = use_depth ? 1 : 0;
  use_normals = use_normals ? 1 : 0;
  OVN_REQUIRE(!stacked_dev || use_depth + use_normals > 0, OVN_ERR_ARG,
              "ovn_render_scans: stacked output requested with no channel enabled");
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(poses_dev != nullptr, OVN_ERR_ARG, "ovn_render_scans: poses is NULL");
  OVN_REQUIRE(cos_az_dev && sin_az_dev && cos_pitch_dev && sin_pitch_dev, OVN_ERR_ARG, "ovn_render_scans: NULL direction table");
  OVN_ON_DEVICE(ctx->device);
  return ovn_render_scans_forward(ctx, vertices_dev, (int)n_vertices, triangles_dev, (int)n_triangles, bvh_nodes_dev, bvh_order_dev,
                                  (int)bvh_leaves, poses_dev, n_scans, proj_h, proj_w, cos_az_dev, sin_az_dev, cos_pitch_dev,
                                  sin_pitch_dev, max_range, range_dev, tri_id_dev, vertex_dev, normal_dev, stacked_dev, use_depth,
                                  use_normals, (hipStream_t)stream);
}

namespace {
bool tsdf_volume_ok(int nx, int ny, int nz, const double* origin, double voxel) {
  if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny > 2147483647ll || (int64_t)nx * ny * nz > 2147483647ll) return false;
  if (!origin || !(voxel > 0.0) || !((float)voxel > 0.0f) || !std::isfinite((float)voxel)) return false;
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite((float)origin[a])) return false;
  return true;
}

// the window of ovn_tsdf_window_*: dimensions that are multiples of 8 and >= 16, a base of multiples of 8, every index within 2^20
constexpr int WINDOW_MAX_INDEX = 1 << 20;
bool tsdf_window_ok(int nx, int ny, int nz, const int* base, OvnRing* ring) {
  const int n[3] = {nx, ny, nz};
  if (!base) return false;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 16 || n[a] % 8 != 0 || base[a] % 8 != 0) return false;
    if (base[a] < -WINDOW_MAX_INDEX || (int64_t)base[a] + n[a] - 1 > WINDOW_MAX_INDEX) return false;
    const int m = base[a] % n[a];
    ring->base[a] = base[a];
    ring->slot0[a] = m < 0 ? m + n[a] : m;
  }
  return true;
}
#define OVN_WINDOW_TEXT "%s: window %d x %d x %d at base (%d, %d, %d): dimensions and base must be multiples of 8, dimensions >= 16, every " \
                        "index within 2^20"

// ovn_tsdf_integrate (ring NULL) and ovn_tsdf_window_integrate: `fn` names the caller in the messages
int tsdf_integrate_checked(const char* fn, ovn_ctx* ctx, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const double* origin,
                           double voxel, double trunc, double max_weight, const float* range_dev, const double* poses_dev,
                           int64_t n_scans, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg, double max_range,
                           void* stream, const int* base) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "%s: ctx is NULL", fn);
  OVN_REQUIRE(tsdf_dev && weight_dev, OVN_ERR_ARG, "%s: NULL volume buffer", fn);
  OVN_REQUIRE(tsdf_volume_ok(nx, ny, nz, origin, voxel), OVN_ERR_ARG,
              "%s: volume %d x %d x %d (each >= 2, at most 2^31 - 1 samples) needs a finite origin and a voxel > 0", fn, nx, ny, nz);
  OvnRing ring;
  if (base) OVN_REQUIRE(tsdf_window_ok(nx, ny, nz, base, &ring), OVN_ERR_ARG, OVN_WINDOW_TEXT, fn, nx, ny, nz, base[0], base[1], base[2]);
  OVN_REQUIRE((float)trunc > 0.0f && std::isfinite((float)trunc), OVN_ERR_ARG, "%s: trunc must be > 0", fn);
  OVN_REQUIRE((float)max_weight > 0.0f, OVN_ERR_ARG, "%s: max_weight must be > 0", fn);
  OVN_REQUIRE((float)max_range > 0.0f && std::isfinite((float)max_range), OVN_ERR_ARG, "%s: max_range must be > 0", fn);
  OVN_REQUIRE(proj_h >= 1 && proj_w >= 1 && (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "%s: image %d x %d outside 1 .. 2^31 - 1 pixels", fn, proj_h, proj_w);
  OVN_REQUIRE(n_scans >= 0 && n_scans <= 2147483646ll, OVN_ERR_ARG, "%s: bad n_scans %lld", fn, (long long)n_scans);
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(range_dev && poses_dev, OVN_ERR_ARG, "%s: NULL range images or poses", fn);
  OVN_ON_DEVICE(ctx->device);
  return ovn_tsdf_integrate_forward(ctx, tsdf_dev, weight_dev, nx, ny, nz, origin, voxel, trunc, max_weight, range_dev, poses_dev,
                                    (int)n_scans, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, (hipStream_t)stream,
                                    base ? &ring : nullptr);
}
}  // namespace

int ovn_tsdf_integrate(ovn_ctx* ctx, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const double* origin, double voxel,
                       double trunc, double max_weight, const float* range_dev, const double* poses_dev, int64_t n_scans, int proj_h,
                       int proj_w, double fov_up_deg, double fov_down_deg, double max_range, void* stream) {
  return tsdf_integrate_checked("ovn_tsdf_integrate", ctx, tsdf_dev, weight_dev, nx, ny, nz, origin, voxel, trunc, max_weight, range_dev,
                                poses_dev, n_scans, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, stream, nullptr);
}

int ovn_tsdf_window_integrate(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const double* anchor,
                              const int32_t* base, double voxel, double trunc, double max_weight, const float* range_dev,
                              const double* poses_dev, int64_t n_scans, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                              double max_range) {
  OVN_REQUIRE(base != nullptr, OVN_ERR_ARG, "ovn_tsdf_window_integrate: base is NULL");
  return tsdf_integrate_checked("ovn_tsdf_window_integrate", ctx, tsdf_dev, weight_dev, nx, ny, nz, anchor, voxel, trunc, max_weight,
                                range_dev, poses_dev, n_scans, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, stream, base);
}


namespace {
// ovn_tsdf_triangles (base NULL) and ovn_tsdf_window_triangles: `fn` names the caller in the messages
int tsdf_triangles_checked(const char* fn, ovn_ctx* ctx, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                           const double* origin, double voxel, double min_weight, float* triangles_dev, int64_t capacity,
                           int64_t* n_triangles_dev, void* stream, const int* base, const int* box_lo, const int* box_hi) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "%s: ctx is NULL", fn);
  OVN_REQUIRE(tsdf_dev && weight_dev && n_triangles_dev, OVN_ERR_ARG, "%s: NULL buffer", fn);
  OVN_REQUIRE(tsdf_volume_ok(nx, ny, nz, origin, voxel), OVN_ERR_ARG,
              "%s: volume %d x %d x %d (each >= 2, at most 2^31 - 1 samples) needs a finite origin and a voxel > 0", fn, nx, ny, nz);
  OvnRing ring;
  if (base) {
    OVN_REQUIRE(tsdf_window_ok(nx, ny, nz, base, &ring), OVN_ERR_ARG, OVN_WINDOW_TEXT, fn, nx, ny, nz, base[0], base[1], base[2]);
    OVN_REQUIRE(box_lo && box_hi, OVN_ERR_ARG, "%s: NULL box", fn);
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)   // a cell's far corner is its low corner + 1: the low corners end at base + n - 1
      OVN_REQUIRE(box_lo[a] <= box_hi[a] && box_lo[a] >= base[a] && (int64_t)box_hi[a] <= (int64_t)base[a] + n[a] - 1, OVN_ERR_ARG,
                  "%s: cells %d .. %d of axis %d have corners outside the window %d .. %d", fn, box_lo[a], box_hi[a] - 1, a, base[a],
                  base[a] + n[a] - 1);
  }
  OVN_REQUIRE(min_weight == min_weight, OVN_ERR_ARG, "%s: min_weight is NaN", fn);
  OVN_REQUIRE(capacity >= 0, OVN_ERR_ARG, "%s: capacity %lld < 0", fn, (long long)capacity);
  OVN_ON_DEVICE(ctx->device);
  return ovn_tsdf_triangles_forward(ctx, tsdf_dev, weight_dev, nx, ny, nz, origin, voxel, min_weight, triangles_dev, capacity,
                                    n_triangles_dev, (hipStream_t)stream, base ? &ring : nullptr, box_lo, box_hi);
}

// ovn_tsdf_raycast (base NULL) and ovn_tsdf_window_raycast
int tsdf_raycast_checked(const char* fn, ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny,
                         int nz, const double* origin, const int* base, double voxel, double min_weight, const uint8_t* bricks_dev,
                         const double* poses_dev, int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev,
                         const float* sin_az_dev, const float* cos_pitch_dev, const float* sin_pitch_dev, double min_range,
                         double max_range, double step, float* range_dev, float* vertex_dev, float* normal_dev, float* stacked_dev,
                         int use_depth, int use_normals) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "%s: ctx is NULL", fn);
  OVN_REQUIRE(tsdf_dev && weight_dev, OVN_ERR_ARG, "%s: NULL volume buffer", fn);
  OVN_REQUIRE(tsdf_volume_ok(nx, ny, nz, origin, voxel), OVN_ERR_ARG,
              "%s: volume %d x %d x %d (each >= 2, at most 2^31 - 1 samples) needs a finite origin and a voxel > 0", fn, nx, ny, nz);
  OvnRing ring;
  if (base) OVN_REQUIRE(tsdf_window_ok(nx, ny, nz, base, &ring), OVN_ERR_ARG, OVN_WINDOW_TEXT, fn, nx, ny, nz, base[0], base[1], base[2]);
  OVN_REQUIRE(proj_h >= 1 && proj_w >= 1 && (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "%s: image %d x %d outside 1 .. 2^31 - 1 pixels", fn, proj_h, proj_w);
  OVN_REQUIRE(n_scans >= 0 && n_scans <= 2147483647ll, OVN_ERR_ARG, "%s: bad n_scans %lld", fn, (long long)n_scans);
  const float mn = (float)min_range, mx = (float)max_range, st = (float)step;
  OVN_REQUIRE(mn > 0.0f && std::isfinite(mn) && mx > 0.0f && std::isfinite(mx) && st > 0.0f && std::isfinite(st), OVN_ERR_ARG,
              "%s: min_range %g, max_range %g and step %g must be finite and > 0", fn, min_range, max_range, step);
  OVN_REQUIRE(mn < mx, OVN_ERR_ARG, "%s: min_range %g is not below max_range %g", fn, min_range, max_range);
  const long long K = ovn_tsdf_raycast_samples(min_range, max_range, step, OVN_RAYCAST_MAX_SAMPLES);
  OVN_REQUIRE(K <= OVN_RAYCAST_MAX_SAMPLES, OVN_ERR_ARG, "%s: more than 2^20 samples per ray (range %g .. %g, step %g)", fn, min_range,
              max_range, step);
  OVN_REQUIRE(min_weight == min_weight, OVN_ERR_ARG, "%s: min_weight is NaN", fn);
  OVN_REQUIRE(!vertex_dev || aligned16(vertex_dev), OVN_ERR_ARG, "%s: vertex_dev is not 16-byte aligned", fn);
  use_depth = use_depth ? 1 : 0;
  use_normals = use_normals ? 1 : 0;
  OVN_REQUIRE(!stacked_dev || use_depth + use_normals > 0, OVN_ERR_ARG, "%s: stacked output requested with no channel enabled", fn);
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(poses_dev != nullptr, OVN_ERR_ARG, "%s: poses is NULL", fn);
  OVN_REQUIRE(cos_az_dev && sin_az_dev && cos_pitch_dev && sin_pitch_dev, OVN_ERR_ARG, "%s: NULL direction table", fn);
  OVN_ON_DEVICE(ctx->device);
  return ovn_tsdf_raycast_forward(ctx, tsdf_dev, weight_dev, nx, ny, nz, origin, voxel, min_weight, bricks_dev, poses_dev, n_scans,
                                  proj_h, proj_w, cos_az_dev, sin_az_dev, cos_pitch_dev, sin_pitch_dev, min_range, step, (int)K,
                                  range_dev, vertex_dev, normal_dev, stacked_dev, use_depth, use_normals, (hipStream_t)stream,
                                  base ? &ring : nullptr);
}
}  // namespace

int ovn_tsdf_triangles(ovn_ctx* ctx, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz, const double* origin,
                       double voxel, double min_weight, float* triangles_dev, int64_t capacity, int64_t* n_triangles_dev, void* stream) {
  return tsdf_triangles_checked("ovn_tsdf_triangles", ctx, tsdf_dev, weight_dev, nx, ny, nz, origin, voxel, min_weight, triangles_dev,
                                capacity, n_triangles_dev, stream, nullptr, nullptr, nullptr);
}

int ovn_tsdf_window_triangles(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                              const double* anchor, const int32_t* base, double voxel, double min_weight, const int32_t* box_lo,
                              const int32_t* box_hi, float* triangles_dev, int64_t capacity, int64_t* n_triangles_dev) {
  OVN_REQUIRE(base != nullptr, OVN_ERR_ARG, "ovn_tsdf_window_triangles: base is NULL");
  return tsdf_triangles_checked("ovn_tsdf_window_triangles", ctx, tsdf_dev, weight_dev, nx, ny, nz, anchor, voxel, min_weight,
                                triangles_dev, capacity, n_triangles_dev, stream, base, box_lo, box_hi);
}

int ovn_tsdf_raycast(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                     const double* origin, double voxel, double min_weight, const uint8_t* bricks_dev, const double* poses_dev,
                     int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev, const float* sin_az_dev,
                     const float* cos_pitch_dev, const float* sin_pitch_dev, double min_range, double max_range, double step,
                     float* range_dev, float* vertex_dev, float* normal_dev, float* stacked_dev, int use_depth, int use_normals) {
  return tsdf_raycast_checked("ovn_tsdf_raycast", ctx, stream, tsdf_dev, weight_dev, nx, ny, nz, origin, nullptr, voxel, min_weight,
                              bricks_dev, poses_dev, n_scans, proj_h, proj_w, cos_az_dev, sin_az_dev, cos_pitch_dev, sin_pitch_dev,
                              min_range, max_range, step, range_dev, vertex_dev, normal_dev, stacked_dev, use_depth, use_normals);
}

int ovn_tsdf_window_raycast(ovn_ctx* ctx, void* stream, const float* tsdf_dev, const float* weight_dev, int nx, int ny, int nz,
                            const double* anchor, const int32_t* base, double voxel, double min_weight, const uint8_t* bricks_dev,
                            const double* poses_dev, int64_t n_scans, int proj_h, int proj_w, const float* cos_az_dev,
                            const float* sin_az_dev, const float* cos_pitch_dev, const float* sin_pitch_dev, double min_range,
                            double max_range, double step, float* range_dev, float* vertex_dev, float* normal_dev, float* stacked_dev,
                            int use_depth, int use_normals) {
  OVN_REQUIRE(base != nullptr, OVN_ERR_ARG, "ovn_tsdf_window_raycast: base is NULL");
  return tsdf_raycast_checked("ovn_tsdf_window_raycast", ctx, stream, tsdf_dev, weight_dev, nx, ny, nz, anchor, base, voxel, min_weight,
                              bricks_dev, poses_dev, n_scans, proj_h, proj_w, cos_az_dev, sin_az_dev, cos_pitch_dev, sin_pitch_dev,
                              min_range, max_range, step, range_dev, vertex_dev, normal_dev, stacked_dev, use_depth, use_normals);
}

int ovn_tsdf_window_shift(ovn_ctx* ctx, void* stream, float* tsdf_dev, float* weight_dev, int nx, int ny, int nz, const int32_t* old_base,
                          const int32_t* new_base) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_tsdf_window_shift: ctx is NULL");
  OVN_REQUIRE(tsdf_dev && weight_dev && old_base && new_base, OVN_ERR_ARG, "ovn_tsdf_window_shift: NULL buffer or base");
  OVN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny <= 2147483647ll && (int64_t)nx * ny * nz <= 2147483647ll, OVN_ERR_ARG,
              "ovn_tsdf_window_shift: volume %d x %d x %d (each >= 2, at most 2^31 - 1 samples)", nx, ny, nz);
  OvnRing ring;
  for (const int32_t* base : {old_base, new_base})
    OVN_REQUIRE(tsdf_window_ok(nx, ny, nz, base, &ring), OVN_ERR_ARG, OVN_WINDOW_TEXT, "ovn_tsdf_window_shift", nx, ny, nz, base[0],
                base[1], base[2]);
  OVN_ON_DEVICE(ctx->device);
  return ovn_tsdf_window_shift_forward(tsdf_dev, weight_dev, nx, ny, nz, old_base, new_base, (hipStream_t)stream);
}

int ovn_tsdf_bricks(ovn_ctx* ctx, void* stream, const float* weight_dev, int nx, int ny, int nz, double min_weight,
                    uint8_t* bricks_dev) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_tsdf_bricks: ctx is NULL");
  OVN_REQUIRE(weight_dev && bricks_dev, OVN_ERR_ARG, "ovn_tsdf_bricks: NULL buffer");
  OVN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny <= 2147483647ll && (int64_t)nx * ny * nz <= 2147483647ll, OVN_ERR_ARG,
              "ovn_tsdf_bricks: volume %d x %d x %d (each >= 2, at most 2^31 - 1 samples)", nx, ny, nz);
  OVN_REQUIRE(min_weight == min_weight, OVN_ERR_ARG, "ovn_tsdf_bricks: min_weight is NaN");
  OVN_ON_DEVICE(ctx->device);
  return ovn_tsdf_bricks_forward(weight_dev, nx, ny, nz, min_weight, bricks_dev, (hipStream_t)stream);
}

int ovn_gt_range_images(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans,
                        int64_t max_points_per_scan, const double* ref_poses_dev, const double* inv_cur_pose_dev, int proj_h,
                        int proj_w, double fov_up_deg, double fov_down_deg, double max_range, float* range_dev, void* stream) {
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_gt_range_images: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_gt_range_images: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0 && proj_h > 0 && proj_w > 0 && max_points_per_scan >= 0, OVN_ERR_ARG, "ovn_gt_range_images: bad sizes");
  if (n_scans == 0) return OVN_OK;
  OVN_REQUIRE(offsets_dev && range_dev && (points_dev || max_points_per_scan == 0), OVN_ERR_ARG, "ovn_gt_range_images: NULL buffer");
  OVN_REQUIRE(n_scans <= 65535, OVN_ERR_ARG, "ovn_gt_range_images: at most 65535 scans per call");
  OVN_ON_DEVICE(ctx->device);
  return ovn_gt_range_forward(points_dev, offsets_dev, n_scans, max_points_per_scan, ref_poses_dev, inv_cur_pose_dev, proj_h,
                              proj_w, fov_up_deg, fov_down_deg, max_range, range_dev, (hipStream_t)stream);
}

int ovn_gt_overlap_counts(ovn_ctx* ctx, const float* ref_ranges_dev, const float* cur_range_dev, int n_scans, int proj_h,
                          int proj_w, int32_t* counts_dev, void* stream) {
  OVN_REQUIRE(proj_h <= 0 || proj_w <= 0 || (int64_t)proj_h * proj_w <= 2147483647ll, OVN_ERR_ARG,
              "ovn_gt_overlap_counts: %d x %d pixels per image, at most 2^31 - 1 (H*W)", proj_h, proj_w);
  OVN_REQUIRE(n_scans <= 2147483646, OVN_ERR_ARG, "ovn_gt_overlap_counts: %d scans, at most 2^31 - 2 (one workgroup each and one more)",
              n_scans);
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_gt_overlap_counts: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0 && proj_h > 0 && proj_w > 0, OVN_ERR_ARG, "ovn_gt_overlap_counts: bad sizes");
  OVN_REQUIRE(cur_range_dev && counts_dev && (ref_ranges_dev || n_scans == 0), OVN_ERR_ARG, "ovn_gt_overlap_counts: NULL buffer");
  OVN_ON_DEVICE(ctx->device);
  return ovn_gt_count_forward(ref_ranges_dev, cur_range_dev, n_scans, proj_h * proj_w, counts_dev, (hipStream_t)stream);
}

int ovn_gt_pair_counts(ovn_ctx* ctx, const float* points_dev, const int64_t* offsets_dev, int n_scans, const double* poses_dev,
                       const double* inv_poses_dev, const float* cur_ranges_dev, const int32_t* frame_idx_dev, int n_frames,
                       const int32_t* ref_idx_dev, int n_refs, int proj_h, int proj_w, double fov_up_deg, double fov_down_deg,
                       double max_range, int32_t* counts_dev, void* stream) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_gt_pair_counts: ctx is NULL");
  OVN_REQUIRE(n_scans >= 0 && n_frames >= 0 && n_refs >= 0 && proj_h > 0 && proj_w > 0, OVN_ERR_ARG,
              "ovn_gt_pair_counts: bad sizes");
  OVN_REQUIRE((long long)proj_h * proj_w <= 262144, OVN_ERR_ARG,
              "ovn_gt_pair_counts: %d x %d pixels need %lld bytes of LDS for the two bit planes, 65536 at the most (H*W <= 262144)",
              proj_h, proj_w, 8ll * (((long long)proj_h * proj_w + 31) / 32));
  OVN_REQUIRE((long long)n_frames * n_refs <= 2147483647ll, OVN_ERR_ARG,
              "ovn_gt_pair_counts: %d frames x %d references exceed the grid (2^31 - 1 pairs per call)", n_frames, n_refs);
  if (n_frames == 0 || n_refs == 0) return OVN_OK;
  OVN_REQUIRE(counts_dev != nullptr, OVN_ERR_ARG, "ovn_gt_pair_counts: counts is NULL");
  OVN_REQUIRE(n_scans > 0 && offsets_dev && poses_dev && inv_poses_dev && cur_ranges_dev, OVN_ERR_ARG,
              "ovn_gt_pair_counts: NULL buffer");
  OVN_REQUIRE((frame_idx_dev || n_frames <= n_scans) && (ref_idx_dev || n_refs <= n_scans), OVN_ERR_ARG,
              "ovn_gt_pair_counts: without an index list at most n_scans (%d) frames / references", n_scans);
  // workgroup order: neighbouring pairs share the reference scan (frame fastest, the default: DESIGN.md 22) or the frame's image
  int frame_fastest = 1;
  if (const char* e = getenv("OVN_GT_PAIR_ORDER")) frame_fastest = e[0] == 'r' ? 0 : 1;
  OVN_ON_DEVICE(ctx->device);
  return ovn_gt_pair_forward(points_dev, offsets_dev, n_scans, poses_dev, inv_poses_dev, cur_ranges_dev, frame_idx_dev, n_frames,
                             ref_idx_dev, n_refs, proj_h, proj_w, fov_up_deg, fov_down_deg, max_range, frame_fastest, counts_dev,
                             (hipStream_t)stream);
}

int ovn_set_head_precision(ovn_ctx* ctx, int mode) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_head_precision: ctx is NULL");
  OVN_REQUIRE(mode >= 0 && mode <= 2, OVN_ERR_ARG, "ovn_set_head_precision: mode %d (0 = fp32 MFMA, 1 = f16x3 MFMA, 2 = bf16x3 MFMA)", mode);
  ctx->head_mode = mode;
  return OVN_OK;
}

int ovn_set_head_width_split(ovn_ctx* ctx, int on) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_head_width_split: ctx is NULL");
  OVN_REQUIRE(on == 0 || on == 1, OVN_ERR_ARG, "ovn_set_head_width_split: %d (0 = exact fp32 at widths other than 360, 1 = f16x3 there)", on);
  ctx->head_width_split = on;
  return OVN_OK;
}

int ovn_get_head_width_split(ovn_ctx* ctx, int* on) {
  OVN_REQUIRE(ctx != nullptr && on != nullptr, OVN_ERR_ARG, "ovn_get_head_width_split: NULL argument");
  *on = ctx->head_width_split;
  return OVN_OK;
}

int ovn_set_corr_normalization(ovn_ctx* ctx, int mode) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_corr_normalization: ctx is NULL");
  OVN_REQUIRE(mode >= 0 && mode <= 3, OVN_ERR_ARG,
              "ovn_set_corr_normalization: mode %d (0 = none, 1 = euclidean, 2 = scaling, 3 = standardization)", mode);
  ctx->corr_norm = mode;
  return OVN_OK;
}

int ovn_get_corr_normalization(ovn_ctx* ctx, int* mode) {
  OVN_REQUIRE(ctx != nullptr && mode != nullptr, OVN_ERR_ARG, "ovn_get_corr_normalization: NULL argument");
  *mode = ctx->corr_norm;
  return OVN_OK;
}

int ovn_set_head_compaction(ovn_ctx* ctx, int on) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_head_compaction: ctx is NULL");
  OVN_REQUIRE(on == 0 || on == 1, OVN_ERR_ARG, "ovn_set_head_compaction: %d (0 = walk all 128 channels, 1 = drop the query's dead channels)", on);
  ctx->head_compact = on;
  return OVN_OK;
}

int ovn_set_projection_trig(ovn_ctx* ctx, int mode) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_projection_trig: ctx is NULL");
  OVN_REQUIRE(mode == 0 || mode == 1, OVN_ERR_ARG, "ovn_set_projection_trig: mode %d (0 = NumPy / SVML float32, 1 = correctly rounded)", mode);
  ctx->proj_trig = mode;
  return OVN_OK;
}

int ovn_set_leg_precision(ovn_ctx* ctx, int mode) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_set_leg_precision: ctx is NULL");
  OVN_REQUIRE(mode == 0 || mode == 1, OVN_ERR_ARG, "ovn_set_leg_precision: mode %d (0 = fp32 MFMA, 1 = f16x3 MFMA)", mode);
  if (mode != 0 && ctx->finalized) {   // the rule ovn_finalize applies to a leg registered in f16x3
    const int bad = leg_f16x3_unserved(ctx);
    OVN_REQUIRE(bad < 0, OVN_ERR_ARG, "ovn_set_leg_precision: layer %s: fewer than 128 output positions per image in leg precision f16x3",
                ctx->leg[bad < 0 ? 0 : bad].name.c_str());
  }
  ctx->leg_mode = mode;
  return OVN_OK;
}

int ovn_profile_begin(ovn_ctx* ctx) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_profile_begin: ctx is NULL");
  for (auto& r : ctx->prof_recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->prof_recs.clear();
  ctx->prof = true;
  return OVN_OK;
}

int ovn_profile_end(ovn_ctx* ctx, double* ms_by_kind, int64_t* launches_by_kind) {
  OVN_REQUIRE(ctx && ms_by_kind && launches_by_kind, OVN_ERR_ARG, "ovn_profile_end: NULL argument");
  OVN_ON_DEVICE(ctx->device);
  ctx->prof = false;
  for (int k = 0; k < OVN_K_COUNT; ++k) {
    ms_by_kind[k] = 0.0;
    launches_by_kind[k] = 0;
  }
  int rc = OVN_OK;
  for (auto& r : ctx->prof_recs) {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(r.b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e != hipSuccess) {
      ovn_set_error("ovn_profile_end: %s", hipGetErrorString(e));
      rc = OVN_ERR_HIP;
    } else {
      ms_by_kind[r.kind] += ms;
      launches_by_kind[r.kind] += 1;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->prof_recs.clear();
  return rc;
}

int ovn_debug_conv(ovn_ctx* ctx, int layer, const float* in_dev, int nb, int h, int w, float* out_dev, void* stream) {
  OVN_REQUIRE(ctx && layer >= 0 && layer < (int)ctx->leg.size(), OVN_ERR_ARG, "ovn_debug_conv: no such leg layer");
  OVN_REQUIRE(in_dev && out_dev && nb >= 0, OVN_ERR_ARG, "ovn_debug_conv: bad buffers");
  OVN_ON_DEVICE(ctx->device);
  int oh = 0, ow = 0;
  if (ctx->leg_mode == 0) return ovn_conv_forward(ctx->leg[layer], in_dev, nb, h, w, out_dev, &oh, &ow, (hipStream_t)stream);
  OVN_REQUIRE(nb <= OVN_LEG_SLICE, OVN_ERR_ARG, "ovn_debug_conv: at most %d images per call", OVN_LEG_SLICE);
  if (!ctx->actmax) OVN_HIP_CHECK(hipMalloc((void**)&ctx->actmax, (size_t)OVN_ACTMAX_SLOTS * OVN_LEG_SLICE * OVN_ACTMAX_STRIDE * sizeof(unsigned)));
  OVN_HIP_CHECK(hipMemsetAsync(ctx->actmax, 0, 2 * (size_t)OVN_LEG_SLICE * OVN_ACTMAX_STRIDE * sizeof(unsigned), (hipStream_t)stream));
  int rc = ovn_absmax_forward(in_dev, nb, (long long)h * w * ctx->leg[layer].cin, ctx->actmax, (hipStream_t)stream);
  if (rc) return rc;
  return ovn_conv_forward_f16x3(ctx->leg[layer], in_dev, nb, h, w, out_dev, &oh, &ow, ctx->actmax, ctx->actmax + (size_t)OVN_LEG_SLICE * OVN_ACTMAX_STRIDE,
                                (hipStream_t)stream);
}

int ovn_debug_head_activations(ovn_ctx* ctx, int64_t n, float* o2_dev, float* o3_dev, void* stream) {
  OVN_REQUIRE(ctx && ctx->dbg_o2 && n >= 0 && n <= ctx->dbg_n, OVN_ERR_STATE,
              "ovn_debug_head_activations: call right after ovn_heads with n <= its (first-chunk) pair count");
  OVN_ON_DEVICE(ctx->device);
  const size_t g = (size_t)ctx->head_g;   // 24 at W = 360; W // 15 at any other width
  if (o2_dev)
    OVN_HIP_CHECK(hipMemcpyAsync(o2_dev, ctx->dbg_o2, (size_t)n * g * g * OVN_C2_OUT * sizeof(float),
                                 hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (o3_dev && ctx->dbg_o3)
    OVN_HIP_CHECK(hipMemcpyAsync(o3_dev, ctx->dbg_o3, (size_t)n * (g - 2) * (g - 2) * OVN_C3_OUT * sizeof(float),
                                 hipMemcpyDeviceToDevice, (hipStream_t)stream));
  else if (o3_dev)  // f16x3 mode: o3 never left the fused kernel -- run it again on the o2 still in scratch, with o3 output
    return ovn_c3_dense_forward(ctx, ctx->dbg_o2, ctx->dbg_o2max, (int)n, ctx->dbg_partial, o3_dev, nullptr, nullptr, nullptr, (hipStream_t)stream);
  return OVN_OK;
}

int ovn_head_walk_stats(ovn_ctx* ctx, int32_t* out16_host, void* stream) {
  OVN_REQUIRE(ctx && out16_host, OVN_ERR_ARG, "ovn_head_walk_stats: NULL argument");
  OVN_ON_DEVICE(ctx->device);
  return ovn_delta_walk_stats(ctx, out16_host, (hipStream_t)stream);
}

int64_t ovn_workspace_bytes(ovn_ctx* ctx) { return ctx ? (int64_t)ctx->ws_bytes : 0; }

int ovn_selftest(ovn_ctx* ctx) {
  OVN_REQUIRE(ctx != nullptr, OVN_ERR_ARG, "ovn_selftest: ctx is NULL");
  OVN_ON_DEVICE(ctx->device);
  return ovn_mfma_selftest(nullptr);
}

}  // extern "C"
