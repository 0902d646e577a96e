// The shape check of the 1x1 convolutions, shared by conv1x1.hip (forward, data gradient) and gen_conv_wgrad.hip (weight
// and bias gradients).  x (B,Cin,H,W); pool 1: y (B,Cout,H,W); pool 2: y (B,Cout,H/2,W/2), torch's floor.
#pragma once

#include "conv_igemm.h"

namespace gfla {

constexpr int kPwPix = 256;        // pixels of the low-resolution map per workgroup: 4 waves x 2 MFMA tiles of 32

struct PwShape {
  int64_t Hout, Wout, OP;          // the output map and its pixels
};

static int pw_check(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act, PwShape *s) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || pool < 1 || pool > 2) return GFLA_ERR_BAD_SHAPE;
  if (pool == 2 && (H < 2 || W < 2 || pre_act)) return GFLA_ERR_BAD_SHAPE;
  // a pixel index plus one workgroup's pixels stays an int
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL - kPwPix || B > 65535 || Cin > kCvMaxC || Cout > kCvMaxC)
    return GFLA_ERR_UNSUPPORTED;
  s->Hout = H / pool;
  s->Wout = W / pool;
  s->OP = s->Hout * s->Wout;
  return GFLA_OK;
}

}  // namespace gfla
