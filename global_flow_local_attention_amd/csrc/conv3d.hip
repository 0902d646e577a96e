// The 3-D convolutions of the video discriminator (base_function.py:43-67 ResBlock3DEncoder) on frames-major activations
// x (B,L,C,H,W): forward and data gradient, the windowed variant of conv_igemm.h.  The weight and bias gradients are in
// gen_conv_wgrad.hip, the pool of the shortcut in avg_pool_frames.hip.
//
// A Conv3d of temporal kernel 3 and temporal stride 1 is, per output sample (b, lo), a 2-D convolution over the 3 C
// channels of frames lo - pt .. lo - pt + 2, which lie contiguous in x; frames outside [0, L) read as zero.  Nothing is
// unfolded or zero-stuffed, and a 16-bit sum is not rounded between the three temporal taps.
//
//   y = bias + conv3d(act(x), w) (+ add)           weights: w.permute(0,2,1,3,4) as (Cout, 3 C, k, k), packed by
//                                                   gfla_gen_conv_pack_weights_<T> with Cin = 3 C
//   grad_x = act'(x) adj(grad_y, w)                sample (b, l) over frames l - (2 - pt) .. l + pt of grad_y, clipped to
//                                                   [0, Lout); weights: row j Cout + co = w[co][.][2 - j], packed by
//                                                   gfla_gen_conv_pack_grad_weights_<T> with Cout' = 3 Cout
#include "conv3d.h"

namespace gfla {

template <typename T>
static int conv3d_fwd(const T *x, const void *wp, const float *bias, const T *add, T *y, int64_t B, int64_t L, int64_t C,
                      int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act, double pre_slope, gfla_stream_t stream) {
  if (!x || !wp || !y) return GFLA_ERR_NULL_POINTER;
  C3Shape s;
  int rc = c3_check(B, L, C, Cout, H, W, geometry, &s);
  if (rc != GFLA_OK) return rc;
  CvTile g;
  int64_t cblocks = 0;
  rc = cv_check(geometry, B * s.Lout, kC3KT * C, Cout, H, W, 0, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(add)) % sizeof(T) != 0)
    return GFLA_ERR_UNSUPPORTED;
  const CvWin win = {(int)L, (int)s.Lout, -s.pt, (int)C};
  auto launch = [&](auto geo) {
    conv_igemm_kernel<T, decltype(geo)::value, kCvGen, 1>
        <<<dim3((unsigned)(g.tilesX * g.tilesY), (unsigned)cblocks, (unsigned)(B * s.Lout)), kBlock,
           2 * (size_t)g.halo * kCvRec, static_cast<hipStream_t>(stream)>>>(
            x, static_cast<const unsigned char *>(wp), bias, add, y, (int)(kC3KT * C), (int)Cout, (int)H, (int)W, (int)g.Hout,
            (int)g.Wout, g.tw_log2, g.WM, g.tilesX, 0, pre_act ? 1 : 0, (float)pre_slope, win);
  };
  if (geometry == 0) launch(std::integral_constant<int, 0>());
  else launch(std::integral_constant<int, 1>());
  return launch_status();
}

template <typename T>
static int conv3d_bwd_data(const T *gy, const T *x, const void *wp, T *gx, int64_t B, int64_t L, int64_t C, int64_t Cout,
                           int64_t H, int64_t W, int geometry, int pre_act, double pre_slope, gfla_stream_t stream) {
  if (!gy || !wp || !gx || (pre_act && !x)) return GFLA_ERR_NULL_POINTER;
  C3Shape s;
  int rc = c3_check(B, L, C, Cout, H, W, geometry, &s);
  if (rc != GFLA_OK) return rc;
  // the adjoint reads grad_y (Hout x Wout) and writes H x W; its tiled map (gen_conv_bwd.hip)
  const int adj = geometry == 0 ? 0 : kCvU2K4;
  CvTile g = cv_tile_of(adj, C, adj == kCvU2K4 ? (H + 1) / 2 : H, adj == kCvU2K4 ? (W + 1) / 2 : W);
  g.Hout = H;
  g.Wout = W;
  int64_t cblocks = 0;
  rc = cv_check_tile(adj, C, g, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(gy)) % sizeof(T) != 0)
    return GFLA_ERR_UNSUPPORTED;
  const CvWin win = {(int)s.Lout, (int)L, -(kC3KT - 1 - s.pt), (int)Cout};
  auto launch = [&](auto geo) {
    conv_igemm_kernel<T, decltype(geo)::value, kCvGrad, 1>
        <<<dim3((unsigned)(g.tilesX * g.tilesY), (unsigned)cblocks, (unsigned)(B * L)), kBlock, 2 * (size_t)g.halo * kCvRec,
           static_cast<hipStream_t>(stream)>>>(gy, static_cast<const unsigned char *>(wp), nullptr, pre_act ? x : nullptr, gx,
                                               (int)(kC3KT * Cout), (int)C, (int)s.Hout, (int)s.Wout, (int)H, (int)W,
                                               g.tw_log2, g.WM, g.tilesX, 0, pre_act ? 1 : 0, (float)pre_slope, win);
  };
  if (adj == 0) launch(std::integral_constant<int, 0>());
  else launch(std::integral_constant<int, kCvU2K4>());
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int gfla_conv3d_out_size(int geometry, int64_t L, int64_t H, int64_t W, int64_t *Lout, int64_t *Hout, int64_t *Wout) {
  if (!Lout || !Hout || !Wout) return GFLA_ERR_NULL_POINTER;
  if (geometry < 0 || geometry > 1 || L <= 0 || H <= 0 || W <= 0 || (geometry == 1 && (L < gfla::kC3KT || H < 2 || W < 2)))
    return GFLA_ERR_BAD_SHAPE;
  *Lout = geometry == 0 ? L : L - (gfla::kC3KT - 1);
  gfla::cv_out_size(geometry, H, W, Hout, Wout);
  return GFLA_OK;
}

#define GFLA_DEF_CONV3D(SFX, T, CT)                                                                                       \
  int gfla_conv3d_fwd_##SFX(const T *x, const void *packed, const float *bias, const T *add, T *y, int64_t B, int64_t L,  \
                            int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act, double pre_slope,   \
                            gfla_stream_t stream) {                                                                       \
    return gfla::conv3d_fwd<CT>(reinterpret_cast<const CT *>(x), packed, bias, reinterpret_cast<const CT *>(add),         \
                                reinterpret_cast<CT *>(y), B, L, C, Cout, H, W, geometry, pre_act, pre_slope, stream);    \
  }                                                                                                                       \
  int gfla_conv3d_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, int64_t B, int64_t L,   \
                                 int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act,                \
                                 double pre_slope, gfla_stream_t stream) {                                                \
    return gfla::conv3d_bwd_data<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), packed_grad,  \
                                     reinterpret_cast<CT *>(grad_x), B, L, C, Cout, H, W, geometry, pre_act, pre_slope,   \
                                     stream);                                                                             \
  }
GFLA_DEF_CONV3D(f32, float, float)
GFLA_DEF_CONV3D(f16, uint16_t, f16_t)
GFLA_DEF_CONV3D(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_CONV3D
}
