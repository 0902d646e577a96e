// The data gradients of the generators' convolutions (gen_conv.hip): the gradient variant of conv_igemm.h on the adjoint
// geometry of each forward, one launch, no atomics.
//
//   grad_x = act'(x) adj(g, w),   act'(x) = x > 0 ? 1 : pre_slope (1 without a pre-activation), read from x as stored
//
//   forward            adjoint                                                    packed from torch's weight as
//   S1K3 zeros         S1K3, taps mirrored, Cin <-> Cout                          [8 - tap][chunk of Cout][Cin][.], transposed
//   S1K3 reflect       the same on the (H+2) x (W+2) padded domain into a float32 workspace, then the fold below
//   S2K4               U2K4: four phases of 2 x 2 taps over the half-resolution grid   [tap][chunk of Cout][Cin][.], transposed
//   T2K3               S2K3: Conv2d(k 3, s 2, p 1) of g, the taps as stored            [tap][chunk of Cout][Cin][.], as stored
//
// The fold of the reflect case: padded row -1 mirrors onto row 1 and padded row H onto row H - 2 (columns likewise), so
// grad_x[i][j] sums grad_p over the rows {i + 1, 0 if i == 1, H + 1 if i == H - 2} x the columns of the same rule, in that
// fixed order, in float32, and is rounded once.
#include "conv_igemm.h"

namespace gfla {

template <typename T>
__global__ __launch_bounds__(kBlock) void gen_conv_fold_kernel(const float *__restrict__ gp, const T *__restrict__ x,
                                                               T *__restrict__ gx, int H, int W, int pre_act, float slope,
                                                               int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int j = (int)(idx % W), i = (int)((idx / W) % H);
  const int64_t bc = idx / W / H;
  const float *p = gp + bc * (int64_t)(H + 2) * (W + 2);
  const int rows[3] = {i + 1, i == 1 ? 0 : -1, i == H - 2 ? H + 1 : -1};
  const int cols[3] = {j + 1, j == 1 ? 0 : -1, j == W - 2 ? W + 1 : -1};
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if (rows[a] >= 0 && cols[b] >= 0) s += p[(int64_t)rows[a] * (W + 2) + cols[b]];
  if (pre_act && !(Num<T>::ld(x + idx) > 0.f)) s *= slope;
  gx[idx] = (T)s;
}

// the adjoint geometry of a forward one, its taps, and how the packer reads torch's weight for it
static void gen_conv_adjoint(int geometry, int *adj, int *transposed, int *mirror) {
  *adj = geometry == 0 ? 0 : geometry == 1 ? kCvU2K4 : kCvS2K3;
  *transposed = geometry != 2;
  *mirror = geometry == 0;
}

template <typename T>
static int gen_conv_pack_grad(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int geometry,
                              gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (geometry < 0 || geometry > 2) return GFLA_ERR_BAD_SHAPE;
  int adj, transposed, mirror;
  gen_conv_adjoint(geometry, &adj, &transposed, &mirror);
  return cv_pack<T>(w, src_type, packed, Cin, Cout, kCvGeo[adj].TAPS, transposed, mirror, stream);   // rows: x's channels
}

template <typename T>
static int gen_conv_bwd_data(const T *gy, const T *x, const void *wp, T *gx, void *ws, int64_t B, int64_t Cin, int64_t Cout,
                             int64_t H, int64_t W, int geometry, int pad_mode, int pre_act, double pre_slope,
                             gfla_stream_t stream) {
  if (!gy || !x || !wp || !gx) return GFLA_ERR_NULL_POINTER;
  CvTile fwd;
  int64_t cblocks = 0;
  int rc = cv_check(geometry, B, Cin, Cout, H, W, pad_mode, &fwd, &cblocks);       // the forward's own limits
  if (rc != GFLA_OK) return rc;
  if (pad_mode == 1 && !ws) return GFLA_ERR_NULL_POINTER;
  int adj, transposed, mirror;
  gen_conv_adjoint(geometry, &adj, &transposed, &mirror);
  // the adjoint reads g (fwd.Hout x fwd.Wout) and writes H x W (reflect: (H+2) x (W+2)); its tiled map
  const int64_t OH = H + 2 * pad_mode, OW = W + 2 * pad_mode;
  CvTile g = cv_tile_of(adj, Cin, adj == kCvU2K4 ? (H + 1) / 2 : OH, adj == kCvU2K4 ? (W + 1) / 2 : OW);
  g.Hout = OH;
  g.Wout = OW;
  rc = cv_check_tile(adj, Cin, g, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  const int64_t total = B * Cin * H * W, fold_blocks = ceil_div(total, kBlock);
  if (pad_mode == 1 && fold_blocks > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  const float slope = (float)pre_slope;
  pre_act = pre_act ? 1 : 0;
  auto launch = [&](auto geo, auto var, T *out, const T *aux) {
    conv_igemm_kernel<T, decltype(geo)::value, decltype(var)::value>
        <<<dim3((unsigned)(g.tilesX * g.tilesY), (unsigned)cblocks, (unsigned)B), kBlock, 2 * (size_t)g.halo * kCvRec,
           static_cast<hipStream_t>(stream)>>>(gy, static_cast<const unsigned char *>(wp), nullptr, aux, out, (int)Cout,
                                               (int)Cin, (int)fwd.Hout, (int)fwd.Wout, (int)OH, (int)OW, g.tw_log2, g.WM,
                                               g.tilesX, 0, pre_act, slope);
  };
  using Grad = std::integral_constant<int, kCvGrad>;
  if (pad_mode == 1) {
    launch(std::integral_constant<int, 0>(), std::integral_constant<int, kCvGradPad>(), static_cast<T *>(ws), nullptr);
    rc = launch_status();
    if (rc != GFLA_OK) return rc;
    gen_conv_fold_kernel<T><<<dim3((unsigned)fold_blocks), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float *>(ws), x, gx, (int)H, (int)W, pre_act, slope, total);
  } else if (adj == 0) {
    launch(std::integral_constant<int, 0>(), Grad(), gx, x);
  } else if (adj == kCvU2K4) {
    launch(std::integral_constant<int, kCvU2K4>(), Grad(), gx, x);
  } else {
    launch(std::integral_constant<int, kCvS2K3>(), Grad(), gx, x);
  }
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_gen_conv_grad_packed_bytes(int64_t Cout, int64_t Cin, int geometry, int elem_size) {
  if (Cout <= 0 || Cin <= 0 || geometry < 0 || geometry > 2 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (Cout > gfla::kCvMaxC || Cin > gfla::kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  int adj, transposed, mirror;
  gfla::gen_conv_adjoint(geometry, &adj, &transposed, &mirror);
  return gfla::cv_packed_elems(Cin, Cout, gfla::kCvGeo[adj].TAPS, gfla::kCvRec / elem_size) * elem_size;
}

#define GFLA_DEF_GEN_CONV_BWD(SFX, T, CT)                                                                                  \
  int gfla_gen_conv_pack_grad_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,          \
                                            int geometry, gfla_stream_t stream) {                                          \
    return gfla::gen_conv_pack_grad<CT>(w, src_type, packed, Cout, Cin, geometry, stream);                                 \
  }                                                                                                                        \
  int gfla_gen_conv_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, void *workspace,       \
                                   int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, \
                                   int pre_act, double pre_slope, gfla_stream_t stream) {                                  \
    return gfla::gen_conv_bwd_data<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), packed_grad, \
                                       reinterpret_cast<CT *>(grad_x), workspace, B, Cin, Cout, H, W, geometry, pad_mode,  \
                                       pre_act, pre_slope, stream);                                                        \
  }
GFLA_DEF_GEN_CONV_BWD(f32, float, float)
GFLA_DEF_GEN_CONV_BWD(f16, uint16_t, f16_t)
GFLA_DEF_GEN_CONV_BWD(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_GEN_CONV_BWD
}
