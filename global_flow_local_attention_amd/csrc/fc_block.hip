// C ABI of the MFMA path of ExtractorAttn's fully_connect_layer (fc_gemm.hip, fc_sample.hip): one call per
// direction, all kernels enqueued on the caller's stream, scratch memory supplied by the caller.
//
// Reference: model/networks/base_function.py:799-807 -- logits = Conv2d(128,k*k,1)(nonlinearity(
// Conv2d(2C,128,k,stride k)(cat(BlockExtractor(target, 0), BlockExtractor(source, flow))))).
#include "fc_gemm.h"

namespace gfla {

static int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// amax slots (uint32 each): max |x| of the tensors that get split into f16 terms
enum { kAmaxSrc = 0, kAmaxTgt = 1, kAmaxW = 2, kAmaxZs = 3, kAmaxZt = 4, kAmaxSlots = 8 };

// the kernel of a convolution of the first FC layer
enum FcConv {
  kConvDirect,     // fc_conv in the split arithmetic of the plan (modes 0-3)
  kConvDirect16,   // fc_conv_f32src: the direct kernel with two f16 terms per operand, split while it stages the float32 maps
  kConvWino32,     // Winograd domain, float32 operands (fc_wino.hip)
  kConvWino16,     // Winograd domain, two-term f16 operands (fc_wino16.hip)
};
// the weight-gradient kernel
enum FcWgrad {
  kWgradDirect32,  // fc_wgrad_f32 partials, reduced by fc_wgrad_reduce
  kWgradDirect16,  // fc_wgrad on the f16-split records into dw_s / dw_t, unscaled by fc_unpack_wgrad
  kWgradWino32,    // Winograd domain, float32 operands; reduced (and transformed back) by fc_wino_wgrad_reduce
  kWgradWino16,    // the same with two-term f16 operands (fc_wino16.hip: fc_wino16_wgrad_kernel)
};
static bool fc_wgrad_wino(FcWgrad w) { return w == kWgradWino32 || w == kWgradWino16; }

// Every kernel choice of the FC entry points.  A pure function of (B, C, H, W, k, mode) -- the forward and the backward of
// one call pair derive the same plan, so the backward reads exactly the weight sets the forward packed.
//
// Mode 5 (round 6, measured per launch at B = 32, tools/probe_modes.py): the DIRECT kernels with two f16 terms per operand and
// three cross products (mode 2's arithmetic, fc_conv_impl.h) beat the Winograd-domain f16 kernel on the k = 5 layer -- forward
// 216 + 189 against 437 us, data gradient 236 + 211 against 527 -- and the float32 Winograd kernel on the k = 3 data gradient
// (58 + 56 against 142; the two-term f16 Winograd kernel took 166); the k = 3 forward stays in the Winograd domain (114
// against 65 + 65).  The SRC32 form of the direct kernel reads the float32 maps every other kernel of the mode uses and splits
// while it stages.  The weight gradients stay in the Winograd domain (k = 5: two-term f16, k = 3: float32): direct 418 + 359 /
// 113 + 95 us.  fc_args_ok guarantees that the direct tiles fit.
struct FcPlan {
  int split;              // f16 terms of the packed records and gradient maps (fc_base_mode): 0 = float32
  bool scaled;            // the kernels read max |x| slots (split modes and mode 5): the forward fills them
  FcConv fwd, dgrad;      // forward / data-gradient convolutions
  // the weight sets the forward packs into the workspace; the backward reads no others
  bool pack_wf, pack_wd;  // direct-kernel packs of the forward / data-gradient convolutions, ...
  int pack_split;         // ... in this split arithmetic
  bool pack_uf, pack_ud;  // Winograd-domain U = G w G^T of the forward (two-term f16 words for kConvWino16) / data gradient
  // mode 4 / 5: the data-gradient convolutions of both halves are issued together (Winograd: one launch), their folds as one
  bool dgrads_together;
  FcWgrad wgrad;          // weight gradient of one half (the per-half entry points, one-sided backward calls)
  FcWgrad wgrad_both;     // ... of both halves as one grid (fc_backward with both input gradients wanted)
  bool wgrads_together;   // that grid is allowed (tuning key 21 = 2: one launch per half)
  // bf16 / f16 features (mode 1) at k = 5: the one-f16-term weight-gradient kernel was this path's slowest (226 us per half at
  // B = 8, 64x64, against ~125 for the Winograd-domain kernel, profiles/r2_face_bf16_kernel_stats.txt); its operands are exact
  // in float32, so the records are unpacked to float32 and the weight gradient runs in the Winograd domain (both halves in one
  // grid: on the two-term f16 kernel, whose max |x| slots the one-f16-term kernels filled)
  bool wgrad_x32;
  // d Gs by owner-computes (fc_sample.hip: fc_scatter_own_kernel) when both gradient maps are wanted and a row of the map fits
  // the LDS: no global atomics, no memset of the source half's map, and max |dz| of both maps as by-products (tuning key 46 =
  // 1: round 2's atomics)
  bool own_scatter;
};

static FcPlan fc_plan(int64_t B, int C, int H, int W, int k, int mode) {
  (void)C;
  FcPlan P;
  P.split = fc_base_mode(mode);
  P.scaled = P.split != 0 || mode == 5;
  P.fwd = mode == 4 ? kConvWino32 : mode == 5 ? (k == 5 ? kConvDirect16 : kConvWino16) : kConvDirect;
  P.dgrad = mode == 4 ? kConvWino32 : mode == 5 ? kConvDirect16 : kConvDirect;
  P.pack_wf = P.fwd == kConvDirect || P.fwd == kConvDirect16;
  P.pack_wd = P.dgrad == kConvDirect || P.dgrad == kConvDirect16;
  P.pack_split = P.dgrad == kConvDirect16 ? 2 : P.split;
  P.pack_uf = P.fwd == kConvWino32 || P.fwd == kConvWino16;
  P.pack_ud = P.dgrad == kConvWino32;
  P.dgrads_together = fc_is_wino(mode);
  P.wgrad_x32 = mode == 1 && k == 5;
  P.wgrad = fc_is_wino(mode) || P.wgrad_x32 ? (mode == 5 && k == 5 ? kWgradWino16 : kWgradWino32)
                                            : (P.split ? kWgradDirect16 : kWgradDirect32);
  P.wgrad_both = P.wgrad_x32 ? kWgradWino16 : P.wgrad;
  P.wgrads_together = tuning(GFLA_TUNE_WINO_LAUNCH) != 2;
  const FcHalf hs = fc_half(H, W, k, true);
  P.own_scatter = tuning(GFLA_TUNE_FC_SCATTER_ATOMICS) != 1 && fc_scatter_own_rows(B, hs.Ho, hs.Wo) >= 1;
  return P;
}

struct FcLayout {
  FcPlan plan;
  FcHalf hs, ht;
  int nch_c, cpad, nt_d, KK, dw1_tiles;
  // forward workspace, kept for backward
  int64_t amax, xs, xt, gs, hid, wd_t, wd_s, gt, wf_t, wf_s, wu_ft, wu_fs, wu_dt, wu_ds, fwd_total;
  // backward scratch: [dzs, dzt, dw_s, dw_t] are zeroed by one memset
  int64_t dzs, dzt, dw_s, dw_t, zero_bytes, zs_pk, zt_pk, dxs, dxt, b0p, dw1p, red, red_tmp, dwp, dwp2, x32, x32b, bwd_total;
};

static FcLayout fc_layout(int64_t B, int C, int H, int W, int k, int mode) {
  const bool wino = fc_is_wino(mode);
  FcLayout L;
  L.plan = fc_plan(B, C, H, W, k, mode);
  const FcPlan &P = L.plan;
  L.hs = fc_half(H, W, k, true);
  L.ht = fc_half(H, W, k, false);
  L.nch_c = (int)ceil_div(C, kFcChunk);
  L.cpad = L.nch_c * kFcChunk;
  L.nt_d = (int)ceil_div(C, kFcTN);
  L.KK = k * k;
  const int nch_h = kFcHidden / kFcChunk;
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += align256(bytes);
    return at;
  };
  L.amax = take(kAmaxSlots * 4);
  L.xs = take(fc_packed_bytes(B, L.nch_c, L.hs.Sx, P.split));
  L.xt = take(fc_packed_bytes(B, L.nch_c, L.ht.Sx, P.split));
  L.gs = take(B * L.hs.Mg * kFcHidden * 4);
  L.hid = take(B * (int64_t)H * W * kFcHidden * 4);
  // (mode 5 sizes the direct forward sets at k = 3 and the Winograd data-gradient sets, which it does not pack, as well: the
  // workspace sizes of round 6 are kept)
  L.wd_t = take(P.pack_wd ? fc_wpack_bytes(L.nt_d, nch_h, k, P.pack_split) : 0);
  L.wd_s = take(P.pack_wd ? fc_wpack_bytes(L.nt_d, nch_h, k, P.pack_split) : 0);
  L.gt = take(B * L.ht.Mg * kFcHidden * 4);
  L.wf_t = take(P.pack_wd ? fc_wpack_bytes(1, L.nch_c, k, P.pack_split) : 0);
  L.wf_s = take(P.pack_wd ? fc_wpack_bytes(1, L.nch_c, k, P.pack_split) : 0);
  // Winograd modes: U = G w G^T of the forward (C -> 128) and data-gradient (128 -> C) convolutions of both halves
  L.wu_ft = take(wino ? fc_wino_wpack_bytes(C, kFcHidden) : 0);
  L.wu_fs = take(wino ? fc_wino_wpack_bytes(C, kFcHidden) : 0);
  L.wu_dt = take(wino ? fc_wino_wpack_bytes(kFcHidden, C) : 0);
  L.wu_ds = take(wino ? fc_wino_wpack_bytes(kFcHidden, C) : 0);
  L.fwd_total = o;

  o = 0;
  L.dzs = take(B * L.hs.Sz * kFcHidden * 4);
  L.dzt = take(B * L.ht.Sz * kFcHidden * 4);
  L.dw_s = take((int64_t)L.KK * L.cpad * kFcHidden * 4);
  L.dw_t = take((int64_t)L.KK * L.cpad * kFcHidden * 4);
  L.zero_bytes = o;
  L.zs_pk = take(P.split ? fc_packed_bytes(B, nch_h, L.hs.Sz, P.split) : 0);
  L.zt_pk = take(P.split ? fc_packed_bytes(B, nch_h, L.ht.Sz, P.split) : 0);
  L.dxs = take(B * L.hs.Mdg * (int64_t)C * 4);
  L.dxt = take(B * L.ht.Mdg * (int64_t)C * 4);
  const int64_t tiles = ceil_div((int64_t)H * W, 64);
  L.b0p = take(B * tiles * kFcHidden * 4);
  // d W1: enough workgroups to fill the chip, few enough rows to reduce
  int t = 1;
  while (B * t < 2 * kNumCU && t * 128 < H * W) t *= 2;
  L.dw1_tiles = t;
  L.dw1p = take(B * t * (32 * kFcHidden + 32) * 4);
  L.red = take((32 * kFcHidden + 32 + kFcHidden) * 4);
  L.red_tmp = take((int64_t)kFcRedTmpFloats * 4);
  // exact-f32 weight gradient: per-split partial sums (the two halves run one after the other and share it)
  const int64_t sp_s = fc_wgrad_splits(B, L.hs.M, L.cpad), sp_t = fc_wgrad_splits(B, L.ht.M, L.cpad);
  int64_t dwp = P.split == 0 ? (sp_s > sp_t ? sp_s : sp_t) * L.KK * L.cpad * kFcHidden * 4 : 0;
  if (fc_wgrad_wino(P.wgrad)) {  // Winograd-domain partials: 36 points per (c, n)
    const int64_t ws_s = fc_wino_wgrad_splits(B, L.hs.Ho, L.hs.Wo, L.cpad, k), ws_t = fc_wino_wgrad_splits(B, L.ht.Ho, L.ht.Wo, L.cpad, k);
    const int64_t w = (ws_s > ws_t ? ws_s : ws_t) * 36 * L.cpad * kFcHidden * 4;
    if (w > dwp) dwp = w;
  }
  L.dwp = take(dwp);
  L.dwp2 = take(dwp);   // the target half's partials: both halves are reduced by one launch pair
  const int64_t x32_s = fc_packed_bytes(B, L.nch_c, L.hs.Sx, 0), x32_t = fc_packed_bytes(B, L.nch_c, L.ht.Sx, 0);
  L.x32 = take(P.wgrad_x32 ? (x32_s > x32_t ? x32_s : x32_t) : 0);
  L.x32b = take(P.wgrad_x32 ? x32_t : 0);   // the target half's copy: both weight gradients run as one grid
  L.bwd_total = o;
  return L;
}

static int fc_args_ok(int64_t B, int64_t C, int64_t H, int64_t W, int k, int mode) {
  if (B < 0 || C <= 0 || H <= 0 || W <= 0 || k < 1) return GFLA_ERR_BAD_SHAPE;
  if (!fc_mode_ok(mode) || (k != 3 && k != 5)) return GFLA_ERR_UNSUPPORTED;
  if (B > 65535 || C > 4096 || H > 2048 || W > 2048) return GFLA_ERR_UNSUPPORTED;
  // the smallest input tile of each convolution (64 outputs + the tap halo) has to fit the LDS of a CU
  const FcHalf hs = fc_half((int)H, (int)W, k, true), ht = fc_half((int)H, (int)W, k, false);
  const int direct = mode == 5 ? 2 : mode;   // mode 5: the direct kernels in mode 2's arithmetic (fc_plan)
  if (mode == 4) {
    if (!fc_wino_fits(hs.Mv, hs.Wo, hs.Wp, k) || !fc_wino_fits(hs.Md, hs.Wp, hs.Wp, k) ||
        !fc_wino_fits(ht.Mv, ht.Wo, ht.Wp, k) || !fc_wino_fits(ht.Md, ht.Wp, ht.Wp, k))
      return GFLA_ERR_UNSUPPORTED;
  } else if (mode == 5) {
    if (!fc_wino16_fits(hs.Mv, hs.Wo, hs.Wp, k) || !fc_wino16_fits(hs.Md, hs.Wp, hs.Wp, k) ||
        !fc_wino16_fits(ht.Mv, ht.Wo, ht.Wp, k) || !fc_wino16_fits(ht.Md, ht.Wp, ht.Wp, k))
      return GFLA_ERR_UNSUPPORTED;
  }
  if (mode != 4 && (!fc_conv_fits(hs.Wo, hs.Wp, k, direct) || !fc_conv_fits(hs.Wp, hs.Wp, k, direct) ||
                    !fc_conv_fits(ht.Wo, ht.Wp, k, direct) || !fc_conv_fits(ht.Wp, ht.Wp, k, direct)))
    return GFLA_ERR_UNSUPPORTED;
  if ((int64_t)64 * (W + 1) * 4 > 64 * 1024) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

#define GFLA_TRY(expr)           \
  do {                           \
    const int rc_ = (expr);      \
    if (rc_ != GFLA_OK) return rc_; \
  } while (0)

// the weight sets of the plan (fc_plan: pack_*), scaled by the slot kAmaxW where the arithmetic splits
static int fc_pack_weight_sets(const FcLayout &L, const float *w0, unsigned char *ws, int C, int k, hipStream_t stream) {
  const FcPlan &P = L.plan;
  const uint32_t *a_w = reinterpret_cast<const uint32_t *>(ws + L.amax) + kAmaxW;
  if (P.pack_wf || P.pack_wd)
    GFLA_TRY(fc_pack_weights(w0, P.pack_split ? a_w : nullptr, P.pack_wf ? ws + L.wf_t : nullptr, P.pack_wf ? ws + L.wf_s : nullptr,
                             P.pack_wd ? ws + L.wd_t : nullptr, P.pack_wd ? ws + L.wd_s : nullptr, C, k, P.pack_split, stream));
  float *u_ft = reinterpret_cast<float *>(ws + L.wu_ft), *u_fs = reinterpret_cast<float *>(ws + L.wu_fs);
  if (P.fwd == kConvWino16) return fc_wino16_pack_weights(w0, a_w, u_ft, u_fs, C, k, stream);
  if (P.pack_uf || P.pack_ud)
    return fc_wino_pack_weights(w0, P.pack_uf ? u_ft : nullptr, P.pack_uf ? u_fs : nullptr,
                                P.pack_ud ? reinterpret_cast<float *>(ws + L.wu_dt) : nullptr,
                                P.pack_ud ? reinterpret_cast<float *>(ws + L.wu_ds) : nullptr, C, k, stream);
  return GFLA_OK;
}

// one or two Winograd-domain convolutions, float32 or two-term f16 operands (amax[j] = the max |x| slot of job j's input)
static int fc_wino_jobs(const WnConvJob *jobs, int njobs, const uint32_t *const *amax, const uint32_t *amax_w, bool w16, int64_t B,
                        int nch, int k, hipStream_t stream) {
  if (!w16) return fc_wino_conv_jobs(jobs, njobs, B, nch, k, stream);
  return fc_wino16_conv_jobs(jobs, njobs, amax, B, nch, k, amax_w, stream);
}

// the forward convolution of the wanted halves (out_s / out_t; NULL: not wanted) on the packed records of the workspace:
// one launch in the Winograd domain, one per half on the direct kernels
static int fc_fwd_convs(const FcLayout &L, const unsigned char *ws, float *out_s, float *out_t, int64_t B, int k,
                        hipStream_t stream) {
  const FcPlan &P = L.plan;
  const uint32_t *amax = reinterpret_cast<const uint32_t *>(ws + L.amax);
  WnConvJob jobs[2];
  const uint32_t *am[2];
  int n = 0;
  for (int h = 0; h < 2; ++h) {
    const bool src = h == 0;
    float *out = src ? out_s : out_t;
    if (!out) continue;
    const FcHalf &g = src ? L.hs : L.ht;
    const PackedDesc X = fc_desc_packed(ws + (src ? L.xs : L.xt), B, L.nch_c, g.Sx, P.split);
    const uint32_t *a_x = amax + (src ? kAmaxSrc : kAmaxTgt);
    const unsigned char *wf = ws + (src ? L.wf_s : L.wf_t);
    if (P.fwd == kConvDirect16) {
      GFLA_TRY(fc_conv_f32src(X, wf, fc_wpack_bytes(1, L.nch_c, k, 2) / 2, out, g.Mg * kFcHidden, kFcHidden, kFcHidden, B, L.nch_c,
                              g.Mv, g.Wo, g.Wp, k, a_x, amax + kAmaxW, stream));
    } else if (P.fwd == kConvDirect) {
      GFLA_TRY(fc_conv(X, wf, fc_wpack_bytes(1, L.nch_c, k, P.split) / fc_nsplit(P.split), out, g.Mg * kFcHidden, kFcHidden,
                       kFcHidden, B, L.nch_c, g.Mv, g.Wo, g.Wp, k, P.split, P.split ? a_x : nullptr,
                       P.split ? amax + kAmaxW : nullptr, stream));
    } else {
      jobs[n] = WnConvJob{X, reinterpret_cast<const float *>(ws + (src ? L.wu_fs : L.wu_ft)), out, g.Mg * kFcHidden, kFcHidden,
                          kFcHidden, g.Mv, g.Wo, g.Wp, g.Sx};
      am[n++] = a_x;
    }
  }
  return n ? fc_wino_jobs(jobs, n, am, amax + kAmaxW, P.fwd == kConvWino16, B, L.nch_c, k, stream) : GFLA_OK;
}

// the data-gradient convolution of the wanted halves from their gradient maps in scratch (packed, for the split modes) into
// dxs / dxt: one launch in the Winograd domain, one per half on the direct kernels
static int fc_dgrad_convs(const FcLayout &L, const unsigned char *ws, unsigned char *sc, bool want_s, bool want_t, int64_t B, int C,
                          int k, hipStream_t stream) {
  const FcPlan &P = L.plan;
  const uint32_t *amax = reinterpret_cast<const uint32_t *>(ws + L.amax);
  const int nch_h = kFcHidden / kFcChunk;
  WnConvJob jobs[2];
  int n = 0;
  for (int h = 0; h < 2; ++h) {
    const bool src = h == 0;
    if (!(src ? want_s : want_t)) continue;
    const FcHalf &g = src ? L.hs : L.ht;
    const float *dz = reinterpret_cast<const float *>(sc + (src ? L.dzs : L.dzt));
    float *dx = reinterpret_cast<float *>(sc + (src ? L.dxs : L.dxt));
    const uint32_t *a_z = amax + (src ? kAmaxZs : kAmaxZt);
    const unsigned char *wd = ws + (src ? L.wd_s : L.wd_t);
    if (P.dgrad == kConvDirect16) {
      GFLA_TRY(fc_conv_f32src(fc_desc_nhwc(dz, g.Sz, kFcHidden), wd, fc_wpack_bytes(L.nt_d, nch_h, k, 2) / 2, dx, g.Mdg * (int64_t)C,
                              C, C, B, nch_h, g.Md, g.Wp, g.Wp, k, a_z, amax + kAmaxW, stream));
    } else if (P.dgrad == kConvDirect) {
      const PackedDesc Z = P.split ? fc_desc_packed(sc + (src ? L.zs_pk : L.zt_pk), B, nch_h, g.Sz, P.split)
                                   : fc_desc_nhwc(dz, g.Sz, kFcHidden);
      GFLA_TRY(fc_conv(Z, wd, fc_wpack_bytes(L.nt_d, nch_h, k, P.split) / fc_nsplit(P.split), dx, g.Mdg * (int64_t)C, C, C, B,
                       nch_h, g.Md, g.Wp, g.Wp, k, P.split, P.split ? a_z : nullptr, P.split ? amax + kAmaxW : nullptr, stream));
    } else {
      jobs[n++] = WnConvJob{fc_desc_nhwc(dz, g.Sz, kFcHidden), reinterpret_cast<const float *>(ws + (src ? L.wu_ds : L.wu_dt)), dx,
                            g.Mdg * (int64_t)C, C, C, g.Md, g.Wp, g.Wp, g.Sz};
    }
  }
  return n ? fc_wino_conv_jobs(jobs, n, B, nch_h, k, stream) : GFLA_OK;
}

// the activation records the weight gradient reads: the workspace's, or their float32 copies in scratch (plan: wgrad_x32)
static PackedDesc fc_wgrad_x(const FcLayout &L, const unsigned char *ws, const unsigned char *sc, bool src, int64_t B) {
  const FcHalf &g = src ? L.hs : L.ht;
  if (L.plan.wgrad_x32) return fc_desc_packed(sc + (src ? L.x32 : L.x32b), B, L.nch_c, g.Sx, 0);
  return fc_desc_packed(ws + (src ? L.xs : L.xt), B, L.nch_c, g.Sx, L.plan.split);
}

// the weight-gradient kernel of one half (plan: wgrad), partial sums into this half's buffer; no reduction
static int fc_wgrad_half(const FcLayout &L, bool src, const unsigned char *ws, unsigned char *sc, int64_t B, int k,
                         hipStream_t stream) {
  const FcPlan &P = L.plan;
  const FcHalf &g = src ? L.hs : L.ht;
  const uint32_t *amax = reinterpret_cast<const uint32_t *>(ws + L.amax);
  const PackedDesc X = fc_wgrad_x(L, ws, sc, src, B);
  const float *dz = reinterpret_cast<const float *>(sc + (src ? L.dzs : L.dzt));
  float *part = reinterpret_cast<float *>(sc + (src ? L.dwp : L.dwp2));
  switch (P.wgrad) {
    case kWgradWino16: {
      const WwJob job{X, dz, part, g.Sz * kFcHidden, g.lead, g.Sx, g.Ho, g.Wo, g.Wp};
      const uint32_t *const ax[1] = {amax + (src ? kAmaxSrc : kAmaxTgt)}, *const az[1] = {amax + (src ? kAmaxZs : kAmaxZt)};
      return fc_wino16_wgrad_jobs(&job, 1, L.cpad, B, k, ax, az, stream);
    }
    case kWgradWino32:
      return fc_wino_wgrad(X, dz, g.Sz * kFcHidden, g.lead, part, L.cpad, B, g.Ho, g.Wo, g.Wp, g.Sx, k, stream);
    case kWgradDirect32:
      return fc_wgrad_f32(X, fc_desc_nhwc(dz, g.Sz, kFcHidden), g.lead, part, L.cpad, B, g.M, g.Wp, k, stream);
    default:
      return fc_wgrad(X, fc_desc_packed(sc + (src ? L.zs_pk : L.zt_pk), B, kFcHidden / kFcChunk, g.Sz, P.split), g.lead,
                      reinterpret_cast<float *>(sc + (src ? L.dw_s : L.dw_t)), L.cpad, B, g.M, g.Wp, k, P.split, stream);
  }
}

// the Winograd-domain weight gradients of both halves as ONE grid (plan: wgrad_both); the max |x| slots of the two-term f16
// kernel are the forward's (activations) and this call's (gradient maps)
static int fc_wgrad_both(const FcLayout &L, const unsigned char *ws, unsigned char *sc, int64_t B, int k, hipStream_t stream) {
  const uint32_t *amax = reinterpret_cast<const uint32_t *>(ws + L.amax);
  const WwJob jobs[2] = {
      {fc_wgrad_x(L, ws, sc, true, B), reinterpret_cast<const float *>(sc + L.dzs), reinterpret_cast<float *>(sc + L.dwp),
       L.hs.Sz * kFcHidden, L.hs.lead, L.hs.Sx, L.hs.Ho, L.hs.Wo, L.hs.Wp},
      {fc_wgrad_x(L, ws, sc, false, B), reinterpret_cast<const float *>(sc + L.dzt), reinterpret_cast<float *>(sc + L.dwp2),
       L.ht.Sz * kFcHidden, L.ht.lead, L.ht.Sx, L.ht.Ho, L.ht.Wo, L.ht.Wp}};
  if (L.plan.wgrad_both == kWgradWino16) {
    const uint32_t *const ax[2] = {amax + kAmaxSrc, amax + kAmaxTgt}, *const az[2] = {amax + kAmaxZs, amax + kAmaxZt};
    return fc_wino16_wgrad_jobs(jobs, 2, L.cpad, B, k, ax, az, stream);
  }
  return fc_wino_wgrad_jobs(jobs, 2, L.cpad, B, k, stream);
}

// source16 / target16 (gfla_fc_forward_f16; source and target are then NULL): float16 features, mode 1 only -- the records
// are packed straight from the f16 maps, unscaled, and only the weights get a max |x| pass
static int fc_forward(const float *source, const float *target, const float *flow, const float *w0, const float *b0,
                      const float *w1, const float *b1, void *ws_, float *logits, int64_t B, int C, int H, int W,
                      int k, float slope, int mode_, hipStream_t stream, const uint16_t *source16 = nullptr,
                      const uint16_t *target16 = nullptr) {
  const bool f16 = source16 != nullptr;
  if (f16 ? !target16 : (!source || !target)) return GFLA_ERR_NULL_POINTER;
  if (!flow || !w0 || !w1 || !ws_ || !logits) return GFLA_ERR_NULL_POINTER;
  if (f16 && mode_ != 1) return GFLA_ERR_UNSUPPORTED;
  GFLA_TRY(fc_args_ok(B, C, H, W, k, mode_));
  if (B == 0) return GFLA_OK;
  note_path(mode_ == 5 ? GFLA_PATH_FC_FWD_MODE5 : GFLA_PATH_FC_FWD_MODE0 + mode_);
  const FcLayout L = fc_layout(B, C, H, W, k, mode_);
  const FcPlan &P = L.plan;
  unsigned char *ws = static_cast<unsigned char *>(ws_);
  uint32_t *amax = reinterpret_cast<uint32_t *>(ws + L.amax);
  if (P.scaled) {   // the f16-split modes scale by max |x|; the float32 modes never read the slots
    if (hipMemsetAsync(amax, 0, kAmaxSlots * 4, stream) != hipSuccess) return GFLA_ERR_LAUNCH;
    if (f16)   // (zero activation slots: scale 1 for every kernel that reads them, forward and backward)
      GFLA_TRY(fc_maxabs(w0, (int64_t)kFcHidden * 2 * C * k * k, amax + kAmaxW, stream));
    else
      GFLA_TRY(fc_maxabs_multi(source, B * (int64_t)C * H * W, amax + kAmaxSrc, target, B * (int64_t)C * H * W, amax + kAmaxTgt,
                               w0, (int64_t)kFcHidden * 2 * C * k * k, amax + kAmaxW, stream));
  }
  GFLA_TRY(fc_pack_weight_sets(L, w0, ws, C, k, stream));
  if (f16)
    GFLA_TRY(fc_pack_act2_f16(source16, ws + L.xs, L.hs, target16, ws + L.xt, L.ht, B, C, H, W, stream));
  else
    GFLA_TRY(fc_pack_act2(source, P.split ? amax + kAmaxSrc : nullptr, ws + L.xs, L.hs, target, P.split ? amax + kAmaxTgt : nullptr,
                          ws + L.xt, L.ht, B, C, H, W, P.split, stream));
  float *gs = reinterpret_cast<float *>(ws + L.gs), *gt = reinterpret_cast<float *>(ws + L.gt);
  GFLA_TRY(fc_fwd_convs(L, ws, gs, gt, B, k, stream));
  return fc_sample_tail_fwd(gs, gt, flow, b0, w1, b1, reinterpret_cast<float *>(ws + L.hid), logits, B, H, W, k,
                            L.hs.Mg * kFcHidden, L.ht.Mg * kFcHidden, L.hs.Wo, L.ht.Wo, slope, stream);
}

// what fc_backward has already done for both halves when it calls fc_half_backward
struct FcHalfCall {
  int acc_x = 0;             // add into g_x
  bool z_ready = false;      // max |dz| and the packed gradient map exist
  bool dgrad_done = false;   // the data-gradient convolution AND its fold are enqueued
  bool fold_later = false;   // fc_backward folds both halves in one launch
  bool wgrad_later = false;  // fc_backward launches both halves' weight gradients as one grid
  bool reduce = true;        // reduce the weight-gradient partials here (false: fc_backward reduces both halves together)
};

// data gradient (transposed convolution + replicate-pad fold) and weight gradient of one half, from its f32
// Z-layout gradient map
static int fc_half_backward(const FcLayout &L, bool source, unsigned char *ws, unsigned char *sc, float *g_x, float *g_w0,
                            int64_t B, int C, int H, int W, int k, const FcHalfCall &call, hipStream_t stream) {
  const FcPlan &P = L.plan;
  const FcHalf &g = source ? L.hs : L.ht;
  uint32_t *amax = reinterpret_cast<uint32_t *>(ws + L.amax);
  uint32_t *a_z = amax + (source ? kAmaxZs : kAmaxZt);
  float *dz = reinterpret_cast<float *>(sc + (source ? L.dzs : L.dzt));
  if (P.split && !call.z_ready) {
    GFLA_TRY(fc_maxabs(dz, B * g.Sz * kFcHidden, a_z, stream));
    GFLA_TRY(fc_pack_z(dz, a_z, sc + (source ? L.zs_pk : L.zt_pk), B, g.Sz, kFcHidden, P.split, stream));
  }
  if (g_x && !call.dgrad_done) {
    // (raises a slot that is zero or already holds the maximum)
    if (P.dgrad == kConvDirect16) GFLA_TRY(fc_maxabs(dz, B * g.Sz * kFcHidden, a_z, stream));
    GFLA_TRY(fc_dgrad_convs(L, ws, sc, source, !source, B, C, k, stream));
    if (!call.fold_later)
      GFLA_TRY(fc_fold(reinterpret_cast<const float *>(sc + (source ? L.dxs : L.dxt)), g_x, B, C, H, W, g, g.Mdg * (int64_t)C,
                       call.acc_x, stream));
  }
  if (!g_w0) return GFLA_OK;
  if (P.wgrad_x32)
    GFLA_TRY(fc_unpack_act(ws + (source ? L.xs : L.xt), amax + (source ? kAmaxSrc : kAmaxTgt),
                           reinterpret_cast<float *>(sc + (source ? L.x32 : L.x32b)), B, L.nch_c, g.Sx, stream));
  if (!call.wgrad_later) {
    if (P.wgrad == kWgradWino16) GFLA_TRY(fc_maxabs(dz, B * g.Sz * kFcHidden, a_z, stream));   // (as above)
    GFLA_TRY(fc_wgrad_half(L, source, ws, sc, B, k, stream));
  }
  if (!call.reduce) return GFLA_OK;
  float *part = reinterpret_cast<float *>(sc + (source ? L.dwp : L.dwp2));
  if (fc_wgrad_wino(P.wgrad))
    return fc_wino_wgrad_reduce(part, fc_wino_wgrad_splits(B, g.Ho, g.Wo, L.cpad, k), g_w0, C, source ? C : 0, L.cpad, k, stream);
  if (P.wgrad == kWgradDirect32)
    return fc_wgrad_reduce(part, fc_wgrad_splits(B, g.M, L.cpad), g_w0, C, source ? C : 0, L.cpad, k, stream);
  return GFLA_OK;   // (kWgradDirect16: fc_unpack_wgrad, by the caller)
}

static int fc_fold_both(const FcLayout &L, const unsigned char *sc, float *g_source, float *g_target, int acc_s, int64_t B, int C,
                        int H, int W, hipStream_t stream) {
  return fc_fold2(reinterpret_cast<const float *>(sc + L.dxs), g_source, L.hs, L.hs.Mdg * (int64_t)C, acc_s,
                  reinterpret_cast<const float *>(sc + L.dxt), g_target, L.ht, L.ht.Mdg * (int64_t)C, 0, B, C, H, W, stream);
}

static int fc_unpack_wgrad_both(const FcLayout &L, const unsigned char *ws, unsigned char *sc, float *g_w0, int C, int k,
                                hipStream_t stream) {
  const uint32_t *a = reinterpret_cast<const uint32_t *>(ws + L.amax);
  return fc_unpack_wgrad(reinterpret_cast<float *>(sc + L.dw_t), reinterpret_cast<float *>(sc + L.dw_s), a + kAmaxTgt, a + kAmaxSrc,
                         a + kAmaxZt, a + kAmaxZs, g_w0, C, L.cpad, k, stream);
}

// (Round 4, measured and dropped: the weight gradients of both halves on a library-owned side stream, forked from and joined
// to the caller's stream with events, concurrently with the data-gradient convolutions and their folds -- 4.75 ms per
// step against 4.66 on one stream, profiles/r4_fc_backward_side_stream.txt.  Both chains are full-chip kernels that own a
// CU's whole register file; side by side they only contend.)
static int fc_backward(void *ws_, const float *flow, const float *w1, const float *g_logits, void *scratch_,
                       float *g_source, float *g_target, float *g_flow, float *g_w0, float *g_b0, float *g_w1,
                       float *g_b1, int64_t B, int C, int H, int W, int k, float slope, int mode_, int flags,
                       hipStream_t stream) {
  if (!ws_ || !flow || !w1 || !g_logits || !scratch_) return GFLA_ERR_NULL_POINTER;
  GFLA_TRY(fc_args_ok(B, C, H, W, k, mode_));
  if (B == 0) return GFLA_OK;
  note_path(mode_ == 5 ? GFLA_PATH_FC_BWD_MODE5 : GFLA_PATH_FC_BWD_MODE0 + mode_);
  const FcLayout L = fc_layout(B, C, H, W, k, mode_);
  const FcPlan &P = L.plan;
  unsigned char *ws = static_cast<unsigned char *>(ws_), *sc = static_cast<unsigned char *>(scratch_);
  uint32_t *amax = reinterpret_cast<uint32_t *>(ws + L.amax);
  const float *hid = reinterpret_cast<const float *>(ws + L.hid);
  float *red_tmp = reinterpret_cast<float *>(sc + L.red_tmp);
  const float *gs = reinterpret_cast<const float *>(ws + L.gs);
  const bool need_s = g_source || g_w0, need_t = g_target || g_w0;
  float *dzs = need_s ? reinterpret_cast<float *>(sc + L.dzs) : nullptr;
  float *dzt = need_t ? reinterpret_cast<float *>(sc + L.dzt) : nullptr;
  float *b0p = g_b0 ? reinterpret_cast<float *>(sc + L.b0p) : nullptr;
  const int64_t tiles = ceil_div((int64_t)H * W, 64);
  const bool own = need_s && need_t && P.own_scatter;
  if (hipMemsetAsync(sc + (own ? L.dzt : 0), 0, L.zero_bytes - (own ? L.dzt : 0), stream) != hipSuccess) return GFLA_ERR_LAUNCH;
  if ((P.scaled || own) && hipMemsetAsync(amax + kAmaxZs, 0, 8, stream) != hipSuccess) return GFLA_ERR_LAUNCH;
  GFLA_TRY(fc_sample_tail_bwd(gs, flow, hid, w1, g_logits, own ? nullptr : dzs, dzt, g_flow, b0p, B, H, W, k, L.hs.Mg * kFcHidden,
                              L.hs.Wo, L.hs.Wp, L.ht.Wp, L.hs.Sz * kFcHidden, L.ht.Sz * kFcHidden, L.hs.lead, L.ht.lead, slope,
                              flags & GFLA_FC_ACCUMULATE_FLOW, stream, own ? amax + kAmaxZt : nullptr));
  if (own)
    GFLA_TRY(fc_sample_scatter_own(flow, dzt, dzs, amax + kAmaxZt, amax + kAmaxZs, B, H, W, k, L.hs.Ho, L.hs.Wo, L.hs.Wp, L.ht.Wp,
                                   L.hs.Sz * kFcHidden, L.ht.Sz * kFcHidden, L.hs.lead, L.ht.lead, L.hs.Sz, stream));
  const float *dw1p = nullptr;
  if (g_w1 || g_b1) {
    float *part = reinterpret_cast<float *>(sc + L.dw1p);
    GFLA_TRY(fc_dw1(hid, g_logits, part, B, H * W, L.KK, L.dw1_tiles, slope, stream));
    dw1p = part;
  }
  // d b0, d W1, d b1: one two-pass reduction that writes all three in place (8 reduce launches + 4 device copies before).
  // (Round 4, measured and dropped: this chain and the forward's weight transform forked onto a library-owned second
  // stream -- 4.449 ms per step against 4.460 on the caller's stream alone, profiles/r4_fc_small_kernels_side_stream.txt.)
  GFLA_TRY(fc_reduce_bias_w1(b0p, B * tiles, g_b0, dw1p, B * L.dw1_tiles, g_w1, g_b1, L.KK, red_tmp, stream));
  const int acc_s = (flags & GFLA_FC_ACCUMULATE_SOURCE) ? 1 : 0;
  const bool both_x = g_source && g_target;
  const bool dgrads_done = P.dgrads_together && both_x;
  if (dgrads_done) {
    if (P.dgrad == kConvDirect16 && !own)   // max |dz| of both gradient maps: the scale of their two-term f16 split
      GFLA_TRY(fc_maxabs_multi(dzs, B * L.hs.Sz * kFcHidden, amax + kAmaxZs, dzt, B * L.ht.Sz * kFcHidden, amax + kAmaxZt, nullptr,
                               0, nullptr, stream));
    GFLA_TRY(fc_dgrad_convs(L, ws, sc, true, true, B, C, k, stream));
    GFLA_TRY(fc_fold_both(L, sc, g_source, g_target, acc_s, B, C, H, W, stream));   // ... and their folds in one launch
  }
  // the weight-gradient partials of both halves are summed (and, in the Winograd domain, transformed back) by ONE launch (pair)
  const bool defer = g_w0 && P.wgrad != kWgradDirect16;
  const bool wgrads_done = defer && fc_wgrad_wino(P.wgrad) && both_x && P.wgrads_together;
  // f16-split modes: max |dz| and the packed gradient maps of both halves by one launch each
  const bool z_both = P.split != 0 && need_s && need_t;
  if (z_both) {
    if (!own)
      GFLA_TRY(fc_maxabs_multi(dzs, B * L.hs.Sz * kFcHidden, amax + kAmaxZs, dzt, B * L.ht.Sz * kFcHidden, amax + kAmaxZt, nullptr,
                               0, nullptr, stream));
    GFLA_TRY(fc_pack_z2(dzs, amax + kAmaxZs, sc + L.zs_pk, L.hs.Sz, dzt, amax + kAmaxZt, sc + L.zt_pk, L.ht.Sz, B, kFcHidden,
                        P.split, stream));
  }
  FcHalfCall call;
  call.z_ready = z_both;
  call.dgrad_done = dgrads_done;
  call.fold_later = both_x;   // (both replicate-pad folds by one launch behind the two data-gradient convolutions)
  call.wgrad_later = wgrads_done;
  call.reduce = !defer;
  if (need_s) {
    call.acc_x = acc_s;
    GFLA_TRY(fc_half_backward(L, true, ws, sc, g_source, g_w0, B, C, H, W, k, call, stream));
  }
  if (need_t) {
    call.acc_x = 0;
    GFLA_TRY(fc_half_backward(L, false, ws, sc, g_target, g_w0, B, C, H, W, k, call, stream));
  }
  if (both_x && !dgrads_done) GFLA_TRY(fc_fold_both(L, sc, g_source, g_target, acc_s, B, C, H, W, stream));
  if (wgrads_done) GFLA_TRY(fc_wgrad_both(L, ws, sc, B, k, stream));
  if (defer) {
    float *part_s = reinterpret_cast<float *>(sc + L.dwp), *part_t = reinterpret_cast<float *>(sc + L.dwp2);
    if (fc_wgrad_wino(P.wgrad))
      GFLA_TRY(fc_wino_wgrad_reduce2(part_s, fc_wino_wgrad_splits(B, L.hs.Ho, L.hs.Wo, L.cpad, k), part_t,
                                     fc_wino_wgrad_splits(B, L.ht.Ho, L.ht.Wo, L.cpad, k), g_w0, C, L.cpad, k, stream));
    else
      GFLA_TRY(fc_wgrad_reduce2(part_s, fc_wgrad_splits(B, L.hs.M, L.cpad), part_t, fc_wgrad_splits(B, L.ht.M, L.cpad), g_w0, C,
                                L.cpad, k, stream));
  }
  if (g_w0 && P.wgrad == kWgradDirect16) GFLA_TRY(fc_unpack_wgrad_both(L, ws, sc, g_w0, C, k, stream));
  return GFLA_OK;
}

}  // namespace gfla

extern "C" {
using namespace gfla;

int gfla_fc_supported(int64_t C, int64_t H, int64_t W, int kernel_size, int mode) {
  return fc_args_ok(1, C, H, W, kernel_size, mode) == GFLA_OK ? 1 : 0;
}

int64_t gfla_fc_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int kernel_size, int mode, int which) {
  if (fc_args_ok(B, C, H, W, kernel_size, mode) != GFLA_OK) return -1;
  const FcLayout L = fc_layout(B, (int)C, (int)H, (int)W, kernel_size, mode);
  return which == 0 ? L.fwd_total : L.bwd_total;
}

int gfla_fc_forward_f32(const float *source, const float *target, const float *flow, const float *w0,
                        const float *b0, const float *w1, const float *b1, void *workspace, float *logits, int64_t B,
                        int64_t C, int64_t H, int64_t W, int kernel_size, double slope, int mode,
                        gfla_stream_t stream) {
  return fc_forward(source, target, flow, w0, b0, w1, b1, workspace, logits, B, (int)C, (int)H, (int)W, kernel_size,
                    (float)slope, mode, static_cast<hipStream_t>(stream));
}

int gfla_fc_forward_f16(const uint16_t *source, const uint16_t *target, const float *flow, const float *w0,
                        const float *b0, const float *w1, const float *b1, void *workspace, float *logits, int64_t B,
                        int64_t C, int64_t H, int64_t W, int kernel_size, double slope, gfla_stream_t stream) {
  return fc_forward(nullptr, nullptr, flow, w0, b0, w1, b1, workspace, logits, B, (int)C, (int)H, (int)W, kernel_size,
                    (float)slope, 1, static_cast<hipStream_t>(stream), source, target);
}

int gfla_fc_backward_f32(void *workspace, const float *flow, const float *w1, const float *grad_logits,
                         void *scratch, float *grad_source, float *grad_target, float *grad_flow, float *grad_w0,
                         float *grad_b0, float *grad_w1, float *grad_b1, int64_t B, int64_t C, int64_t H, int64_t W,
                         int kernel_size, double slope, int mode, int flags, gfla_stream_t stream) {
  return fc_backward(workspace, flow, w1, grad_logits, scratch, grad_source, grad_target, grad_flow, grad_w0, grad_b0,
                     grad_w1, grad_b1, B, (int)C, (int)H, (int)W, kernel_size, (float)slope, mode, flags,
                     static_cast<hipStream_t>(stream));
}

/* ---- pieces of the above, exposed for the parity tests ---- */

/* out[0..11] = Hp, Wp, Ho, Wo, pad_t, pad_l, M, Md, lead, Sx, Sz, Mg;  out[12] = Mdg */
int gfla_fc_geometry(int64_t H, int64_t W, int kernel_size, int is_source, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (H <= 0 || W <= 0 || kernel_size < 1) return GFLA_ERR_BAD_SHAPE;
  const FcHalf g = fc_half((int)H, (int)W, kernel_size, is_source != 0);
  const int64_t v[13] = {g.Hp, g.Wp, g.Ho, g.Wo, g.pad_t, g.pad_l, g.M, g.Md, g.lead, g.Sx, g.Sz, g.Mg, g.Mdg};
  for (int i = 0; i < 13; ++i) out[i] = v[i];
  return GFLA_OK;
}

/* convolved map of one half: out (B, Mg, 128) f32, row m = yo*Wo + xo (gfla_fc_geometry) */
int gfla_fc_conv_fwd_f32(const float *x, const float *w0, int is_source, void *workspace, float *out, int64_t B,
                         int64_t C_, int64_t H_, int64_t W_, int kernel_size, int mode, gfla_stream_t stream_) {
  if (!x || !w0 || !workspace || !out) return GFLA_ERR_NULL_POINTER;
  const int C = (int)C_, H = (int)H_, W = (int)W_, k = kernel_size;
  GFLA_TRY(fc_args_ok(B, C, H, W, k, mode));
  if (B == 0) return GFLA_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const FcLayout L = fc_layout(B, C, H, W, k, mode);
  const FcPlan &P = L.plan;
  const FcHalf &g = is_source ? L.hs : L.ht;
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  uint32_t *amax = reinterpret_cast<uint32_t *>(ws + L.amax);
  uint32_t *a_x = amax + (is_source ? kAmaxSrc : kAmaxTgt);
  if (hipMemsetAsync(amax, 0, kAmaxSlots * 4, stream) != hipSuccess) return GFLA_ERR_LAUNCH;
  if (P.scaled) {
    GFLA_TRY(fc_maxabs(x, B * (int64_t)C * H * W, a_x, stream));
    GFLA_TRY(fc_maxabs(w0, (int64_t)kFcHidden * 2 * C * k * k, amax + kAmaxW, stream));
  }
  GFLA_TRY(fc_pack_act(x, P.split ? a_x : nullptr, ws + (is_source ? L.xs : L.xt), B, C, H, W, g, P.split, stream));
  GFLA_TRY(fc_pack_weight_sets(L, w0, ws, C, k, stream));
  return fc_fwd_convs(L, ws, is_source ? out : nullptr, is_source ? nullptr : out, B, k, stream);
}

/* gradients of one half from its Z-layout gradient map z (B, Sz, 128) f32 (zero outside the data, see
 * gfla_fc_geometry): grad_x (B,C,H,W), grad_w0 (128, 2C, k, k) with the other half zero.  `workspace` must hold the
 * result of gfla_fc_conv_fwd_f32 for the same x / w0 / half. */
int gfla_fc_conv_bwd_f32(const float *z, int is_source, void *workspace, void *scratch, float *grad_x, float *grad_w0,
                         int64_t B, int64_t C_, int64_t H_, int64_t W_, int kernel_size, int mode,
                         gfla_stream_t stream_) {
  if (!z || !workspace || !scratch) return GFLA_ERR_NULL_POINTER;
  const int C = (int)C_, H = (int)H_, W = (int)W_, k = kernel_size;
  GFLA_TRY(fc_args_ok(B, C, H, W, k, mode));
  if (B == 0) return GFLA_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const FcLayout L = fc_layout(B, C, H, W, k, mode);
  const FcHalf &g = is_source ? L.hs : L.ht;
  unsigned char *ws = static_cast<unsigned char *>(workspace), *sc = static_cast<unsigned char *>(scratch);
  uint32_t *amax = reinterpret_cast<uint32_t *>(ws + L.amax);
  if (hipMemsetAsync(sc, 0, L.zero_bytes, stream) != hipSuccess) return GFLA_ERR_LAUNCH;
  if (hipMemsetAsync(amax + kAmaxZs, 0, 8, stream) != hipSuccess) return GFLA_ERR_LAUNCH;
  if (hipMemcpyAsync(sc + (is_source ? L.dzs : L.dzt), z, (size_t)(B * g.Sz * kFcHidden * 4), hipMemcpyDeviceToDevice,
                     stream) != hipSuccess)
    return GFLA_ERR_LAUNCH;
  const bool unpack = L.plan.wgrad == kWgradDirect16;   // writes both halves; the reductions write this half's only
  if (grad_w0 && !unpack &&  // the other half of conv0.weight.grad is zero by contract
      hipMemsetAsync(grad_w0, 0, (size_t)kFcHidden * 2 * C * k * k * 4, stream) != hipSuccess)
    return GFLA_ERR_LAUNCH;
  GFLA_TRY(fc_half_backward(L, is_source != 0, ws, sc, grad_x, grad_w0, B, C, H, W, k, FcHalfCall(), stream));
  if (grad_w0 && unpack) GFLA_TRY(fc_unpack_wgrad_both(L, ws, sc, grad_w0, C, k, stream));
  return GFLA_OK;
}

/* ONE internal kernel of the path, on the state a forward + backward of the same shape left in workspace / scratch:
 * per-kernel timing for bench.py and the profiles (results land in scratch areas the next real call overwrites).
 * which: 0 / 1 convolution forward source / target half, 2 / 3 data-gradient convolution, 4 / 5 weight gradient;
 * modes 4 / 5 only: 6 / 7 / 8 = the forward / data-gradient convolutions / weight gradients of BOTH halves, as the step
 * issues them. */
int gfla_fc_kernel_f32(int which, void *workspace, void *scratch, int64_t B, int64_t C_, int64_t H_, int64_t W_,
                       int kernel_size, int mode, gfla_stream_t stream_) {
  if (!workspace || !scratch) return GFLA_ERR_NULL_POINTER;
  if (which < 0 || which > 8 || (which > 5 && !fc_is_wino(mode))) return GFLA_ERR_BAD_SHAPE;
  const int C = (int)C_, H = (int)H_, W = (int)W_, k = kernel_size;
  GFLA_TRY(fc_args_ok(B, C, H, W, k, mode));
  if (B == 0) return GFLA_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const FcLayout L = fc_layout(B, C, H, W, k, mode);
  unsigned char *ws = static_cast<unsigned char *>(workspace), *sc = static_cast<unsigned char *>(scratch);
  const bool src = which == 6 || which == 7 || (which & 1) == 0, tgt = which > 5 || (which & 1) == 1;
  float *gs = reinterpret_cast<float *>(ws + L.gs), *gt = reinterpret_cast<float *>(ws + L.gt);
  switch (which) {
    case 0: case 1: case 6: return fc_fwd_convs(L, ws, src ? gs : nullptr, tgt ? gt : nullptr, B, k, stream);
    case 2: case 3: case 7: return fc_dgrad_convs(L, ws, sc, src, tgt, B, C, k, stream);
    case 4: case 5: return fc_wgrad_half(L, src, ws, sc, B, k, stream);
    default: return fc_wgrad_wino(L.plan.wgrad_both) ? fc_wgrad_both(L, ws, sc, B, k, stream) : GFLA_ERR_UNSUPPORTED;
  }
}

int gfla_fc_tr_probe(const int16_t *image, int n_halves, const int32_t *offsets, int16_t *out, gfla_stream_t stream) {
  if (!image || !offsets || !out) return GFLA_ERR_NULL_POINTER;
  return fc_tr_probe(image, n_halves, offsets, out, static_cast<hipStream_t>(stream));
}
}
