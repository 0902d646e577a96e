// 3x3 convolution + bias + ReLU of the VGG19 feature extractor (external_function.py:323-444), stride 1, zero padding 1,
// NCHW, and its data gradient: the entry points of the S1K3 geometry of conv_igemm.h in its two VGG variants.
//
//   y[b, co, p] = max(0, bias[co] + sum over ci and the nine taps of x[b, ci, p + tap] w[co, ci, tap])
//   dx          = conv3x3(g [y > 0], w mirrored, Cin <-> Cout)     (the weights are frozen: no weight gradient)
//
// Pack layout 0 (forward) is geometry 0's packing; layout 1 (data gradient) indexes the weight transposed, as T2K3 does,
// with the taps mirrored.
#include "conv_igemm.h"

namespace gfla {

template <typename T>
static int conv3x3_pack(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int layout,
                        gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (layout < 0 || layout > 1) return GFLA_ERR_BAD_SHAPE;
  return cv_pack<T>(w, src_type, packed, layout ? Cin : Cout, layout ? Cout : Cin, 9, layout, layout, stream);
}

template <typename T>
static int conv3x3_fwd(const T *x, const void *wp, const float *bias, T *y, int64_t B, int64_t Cin, int64_t Cout, int64_t H,
                       int64_t W, gfla_stream_t stream) {
  if (!x || !wp || !bias || !y) return GFLA_ERR_NULL_POINTER;
  return cv_run<T, kCvVggFwd>(0, x, wp, bias, nullptr, y, B, Cin, Cout, H, W, 0, 0, 0.f, stream);
}

// the convolved map is the output gradient (Cout channels), the result has Cin
template <typename T>
static int conv3x3_bwd(const T *grad_y, const T *y, const void *wp, T *grad_x, int64_t B, int64_t Cin, int64_t Cout,
                       int64_t H, int64_t W, gfla_stream_t stream) {
  if (!grad_y || !y || !wp || !grad_x) return GFLA_ERR_NULL_POINTER;
  return cv_run<T, kCvVggBwd>(0, grad_y, wp, nullptr, y, grad_x, B, Cout, Cin, H, W, 0, 0, 0.f, stream);
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_conv3x3_packed_bytes(int64_t Cout, int64_t Cin, int layout, int elem_size) {
  if (Cout <= 0 || Cin <= 0 || layout < 0 || layout > 1 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (Cout > gfla::kCvMaxC || Cin > gfla::kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  return gfla::cv_packed_elems(layout ? Cin : Cout, layout ? Cout : Cin, 9, gfla::kCvRec / elem_size) * elem_size;
}

#define GFLA_DEF_CONV3X3(SFX, T, CT)                                                                                       \
  int gfla_conv3x3_relu_fwd_##SFX(const T *x, const void *packed, const float *bias, T *y, int64_t B, int64_t Cin,         \
                                  int64_t Cout, int64_t H, int64_t W, gfla_stream_t stream) {                              \
    return gfla::conv3x3_fwd<CT>(reinterpret_cast<const CT *>(x), packed, bias, reinterpret_cast<CT *>(y), B, Cin, Cout,   \
                                 H, W, stream);                                                                            \
  }                                                                                                                        \
  int gfla_conv3x3_relu_bwd_data_##SFX(const T *grad_y, const T *y, const void *packed_grad, T *grad_x, int64_t B,         \
                                       int64_t Cin, int64_t Cout, int64_t H, int64_t W, gfla_stream_t stream) {            \
    return gfla::conv3x3_bwd<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(y), packed_grad,       \
                                 reinterpret_cast<CT *>(grad_x), B, Cin, Cout, H, W, stream);                              \
  }                                                                                                                        \
  int gfla_conv3x3_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int layout,    \
                                      gfla_stream_t stream) {                                                              \
    return gfla::conv3x3_pack<CT>(w, src_type, packed, Cout, Cin, layout, stream);                                         \
  }
GFLA_DEF_CONV3X3(f32, float, float)
GFLA_DEF_CONV3X3(f16, uint16_t, f16_t)
GFLA_DEF_CONV3X3(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_CONV3X3
}
