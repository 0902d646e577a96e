// The convolutions of the generators' bodies (base_function.py:334-391 EncoderBlock / ResBlock, 508-531 ResBlockDecoder,
// 672-691 Jump), forward: the entry points of the three geometries of conv_igemm.h in its generator variant.  The
// gradients are in gen_conv_bwd.hip (data) and gen_conv_wgrad.hip (weight, bias).
//
//   y = bias + conv(act(x), w) (+ add),   act = identity | LeakyReLU(pre_slope), rounded to T once while it is staged
//
// torch's weight is packed as stored: (Cout, Cin, k, k) of a Conv2d (geometry 0, 1), (Cin, Cout, 3, 3) of a
// ConvTranspose2d (geometry 2, indexed transposed); tap = ky k + kx.
#include "conv_igemm.h"

namespace gfla {

template <typename T>
static int gen_conv_pack(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int geometry,
                         gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (geometry < 0 || geometry > 2) return GFLA_ERR_BAD_SHAPE;
  return cv_pack<T>(w, src_type, packed, Cout, Cin, kCvGeo[geometry].TAPS, geometry == 2, 0, stream);
}

template <typename T>
static int gen_conv_fwd(const T *x, const void *wp, const float *bias, const T *add, T *y, int64_t B, int64_t Cin,
                        int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, int pre_act, double pre_slope,
                        gfla_stream_t stream) {
  if (!x || !wp || !y) return GFLA_ERR_NULL_POINTER;
  return cv_run<T, kCvGen>(geometry, x, wp, bias, add, y, B, Cin, Cout, H, W, pad_mode, pre_act ? 1 : 0, (float)pre_slope,
                           stream);
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_gen_conv_packed_bytes(int64_t Cout, int64_t Cin, int geometry, int elem_size) {
  if (Cout <= 0 || Cin <= 0 || geometry < 0 || geometry > 2 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (Cout > gfla::kCvMaxC || Cin > gfla::kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  return gfla::cv_packed_elems(Cout, Cin, gfla::kCvGeo[geometry].TAPS, gfla::kCvRec / elem_size) * elem_size;
}

int gfla_gen_conv_out_size(int geometry, int64_t H, int64_t W, int64_t *Hout, int64_t *Wout) {
  if (!Hout || !Wout) return GFLA_ERR_NULL_POINTER;
  if (geometry < 0 || geometry > 2 || H <= 0 || W <= 0 || (geometry == 1 && (H < 2 || W < 2))) return GFLA_ERR_BAD_SHAPE;
  gfla::cv_out_size(geometry, H, W, Hout, Wout);
  return GFLA_OK;
}

int gfla_gen_conv_geometry(int geometry, int64_t Cout, int64_t H, int64_t W, int elem_size, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  gfla::CvTile g;
  int64_t cblocks = 0;
  const int rc = gfla::cv_check(geometry, 1, 1, Cout, H, W, 0, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  out[0] = (int64_t)1 << g.tw_log2;
  out[1] = g.TH;
  out[2] = g.WM;
  out[3] = g.tilesX;
  out[4] = g.tilesY;
  out[5] = cblocks;
  out[6] = g.halo;
  out[7] = 2 * (int64_t)g.halo * gfla::kCvRec;
  return GFLA_OK;
}

#define GFLA_DEF_GEN_CONV(SFX, T, CT)                                                                                      \
  int gfla_gen_conv_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int geometry, \
                                       gfla_stream_t stream) {                                                             \
    return gfla::gen_conv_pack<CT>(w, src_type, packed, Cout, Cin, geometry, stream);                                      \
  }                                                                                                                        \
  int gfla_gen_conv_fwd_##SFX(const T *x, const void *packed, const float *bias, const T *add, T *y, int64_t B,            \
                              int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, int pre_act,    \
                              double pre_slope, gfla_stream_t stream) {                                                    \
    return gfla::gen_conv_fwd<CT>(reinterpret_cast<const CT *>(x), packed, bias, reinterpret_cast<const CT *>(add),        \
                                  reinterpret_cast<CT *>(y), B, Cin, Cout, H, W, geometry, pad_mode, pre_act, pre_slope,   \
                                  stream);                                                                                 \
  }
GFLA_DEF_GEN_CONV(f32, float, float)
GFLA_DEF_GEN_CONV(f16, uint16_t, f16_t)
GFLA_DEF_GEN_CONV(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_GEN_CONV
}
