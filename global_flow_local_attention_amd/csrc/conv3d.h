// The shape check of the frames-major 3-D convolutions, shared by conv3d.hip (forward, data gradient) and
// gen_conv_wgrad.hip (weight and bias gradients).  x (B,L,C,H,W); y (B,Lout,Cout,Hout,Wout).
//
//   geometry 0  k333  Conv3d(k (3,3,3), s 1, p (1,1,1))            Lout = L      the 2-D geometry S1K3 per frame window
//   geometry 1  k344  Conv3d(k (3,4,4), s (1,2,2), p (0,1,1))      Lout = L - 2  the 2-D geometry S2K4 per frame window
//
// Sample (b, lo) of y is the 2-D convolution of the kC3KT C channels of frames lo - pt .. lo - pt + 2 (conv_igemm.h's
// window): the 2-D family's limits hold for a batch of B Lout (the data gradient: B L) samples of 3 C channels.
#pragma once

#include "conv_igemm.h"

namespace gfla {

constexpr int kC3KT = 3;           // frames of a window: the temporal kernel size of both geometries

struct C3Shape {
  int64_t Lout, Hout, Wout;
  int pt;                          // temporal padding
};

static int c3_check(int64_t B, int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, C3Shape *s) {
  if (B <= 0 || L <= 0 || C <= 0 || Cout <= 0 || H <= 0 || W <= 0 || geometry < 0 || geometry > 1) return GFLA_ERR_BAD_SHAPE;
  if (geometry == 1 && (L < kC3KT || H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  s->pt = geometry == 0 ? 1 : 0;
  s->Lout = L + 2 * s->pt - (kC3KT - 1);
  if (L > 65535 || B * L > 65535 || kC3KT * C > kCvMaxC || kC3KT * Cout > kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  CvTile g;
  int64_t cblocks = 0;
  const int rc = cv_check(geometry, B * s->Lout, kC3KT * C, Cout, H, W, 0, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  s->Hout = g.Hout;
  s->Wout = g.Wout;
  return GFLA_OK;
}

}  // namespace gfla
