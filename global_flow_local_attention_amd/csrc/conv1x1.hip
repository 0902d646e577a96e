// The 1x1 convolutions of the discriminators (the pooled shortcut of ResBlockEncoder, the final Conv2d(C, 1, 1)) and of the
// generator's ResBlock shortcut on the gfx950 matrix cores: forward and data gradient.  The weight and bias gradients are
// the KW = 1 instantiation of gen_conv_wgrad.hip.
//
//   y  = bias + conv1x1(p, w),   p = avg_pool2d(x, 2, 2) (pool 2) | leaky_relu(x, slope) | x (pool 1)
//   dx[b][ci][2i + a][2j + c] = 0.25 sum_co w[co][ci] g[b][co][i][j]      (pool 2; an odd trailing row / column: zero)
//   dx = act'(x) sum_co w[co][ci] g,   act'(x) = x > 0 ? 1 : slope       (pool 1)
//
// GEMM view as in conv_igemm.h: rows = the result's channels, columns = pixels, one chunk of CK reduced channels per MFMA
// step, a pixel of a chunk a 32-byte record in LDS, the weights packed by cv_pack with one tap.  There is one tap and no
// halo, so the tiled map -- the LOW-resolution map in all four cases: y for the forward, g for the gradients -- is walked
// as a flat run of pixels: a workgroup (4 waves) owns 256 consecutive ones of one sample and 64 result channels, a wave
// 2 channel tiles x 2 pixel tiles of 32.  Thread t stages the record of pixel t of the run: two ds_write_b128 per chunk.
// With pool 2 the forward builds the record from the 2 x 2 block while it stages it: four global reads per channel, the
// float32 sum in torch's order ((x00 + x01) + x10) + x11, times 0.25, rounded to T once -- what F.avg_pool2d hands on.
// The pooled data gradient writes the four elements of the block from the lane that holds the low-resolution pixel, and
// the lanes of the last column / row write the zero column / row of an odd W / H: every element of dx is written, by
// exactly one lane, so dx may be uninitialised and nothing is cleared beforehand.
//
// The reduction order per element is chunk ascending, then the k of the MFMA.  No atomics.
#include "conv1x1.h"

namespace gfla {

constexpr int kPwNB = 2;           // 32-pixel MFMA tiles per wave

// in: the staged map, (B,K,H,W) for the forward (x), (B,K,Hout,Wout) for a gradient (g); wp: packed [chunk][M padded to
// 32][CK]; bias: M float32 or NULL (forward only); x: the forward's input, read by the pool 1 gradient with pre_act; out:
// (B,M,Hout,Wout) for the forward, (B,M,H,W) for a gradient
template <typename T, int POOL, bool GRAD>
__global__ __launch_bounds__(kBlock, 2) void conv1x1_kernel(const T *__restrict__ in, const unsigned char *__restrict__ wp,
                                                            const float *__restrict__ bias, const T *__restrict__ x,
                                                            T *__restrict__ out, int K, int M, int H, int W, int Hout,
                                                            int Wout, int pre_act, float slope) {
  constexpr int CK = cv_ck<T>(), MB = kCvMB, NB = kPwNB;
  static_assert(kPwPix == kBlock && kPwPix == 4 * NB * 32, "one staged record per thread, two pixel tiles per wave");
  __shared__ __attribute__((aligned(16))) unsigned char pw_smem[2 * kPwPix * kCvRec];   // [2][pixel][32 bytes]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
  const int OP = Hout * Wout, p0 = blockIdx.x * kPwPix;
  const int64_t plane = (int64_t)H * W;
  const int64_t iplane = GRAD ? (int64_t)OP : plane, oplane = GRAD ? plane : (int64_t)OP;
  const T *ib = in + (int64_t)blockIdx.z * K * iplane;
  const int NCH = (K + CK - 1) / CK, MP = (M + 31) / 32 * 32;

  // the record this thread stages per chunk: pixel p0 + t of the low-resolution map
  int goff = -1;
  if (p0 + t < OP) {
    if constexpr (!GRAD && POOL == 2) {
      const int oy = (p0 + t) / Wout, ox = (p0 + t) - oy * Wout;
      goff = 2 * oy * W + 2 * ox;                                              // the block's first element
    } else {
      goff = p0 + t;
    }
  }
  auto element = [&](int c) -> uint32_t {
    if (c >= K) return 0u;
    const T *p = ib + (int64_t)c * iplane + goff;
    if constexpr (!GRAD && POOL == 2) {
      const float s = Num<T>::ld(p) + Num<T>::ld(p + 1) + Num<T>::ld(p + W) + Num<T>::ld(p + W + 1);
      const T a = (T)(s * 0.25f);                                              // rounded to T once, as torch hands it on
      return cv_bits<T>(&a);
    }
    if constexpr (!GRAD && POOL == 1) {
      if (pre_act) {
        const float v = Num<T>::ld(p);
        const T a = (T)(v > 0.f ? v : v * slope);
        return cv_bits<T>(&a);
      }
    }
    return cv_bits<T>(p);
  };
  uint32_t val[8];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint32_t v = 0u;
      if (goff >= 0) {
        if constexpr (sizeof(T) == 2) v = element(ch * CK + 2 * q) | (element(ch * CK + 2 * q + 1) << 16);
        else v = element(ch * CK + q);
      }
      val[q] = v;
    }
  };
  auto stage = [&](int buf) {
    uint4 *rec = reinterpret_cast<uint4 *>(pw_smem + (buf * kPwPix + t) * kCvRec);
    rec[0] = make_uint4(val[0], val[1], val[2], val[3]);
    rec[1] = make_uint4(val[4], val[5], val[6], val[7]);
  };

  cv_f32x16 acc[MB][NB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // B operand: column l31 of pixel tile wave * NB + j; A operand: row l31 of channel tile cb[i], tiles beyond the padded
  // channel count skipped (wave-uniform)
  int boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) boff[j] = ((wave * NB + j) * 32 + l31) * kCvRec + kh * 16;
  int cb[MB];
  bool mv[MB];
  const unsigned char *wa[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    cb[i] = blockIdx.y * MB + i;
    mv[i] = cb[i] * 32 < MP;
    wa[i] = wp + (int64_t)(mv[i] ? cb[i] * 32 + l31 : 0) * kCvRec + kh * 16;
  }
  const int64_t wstep = (int64_t)MP * kCvRec;   // bytes of one chunk

  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) fetch(ch + 1);
    const unsigned char *Bs = pw_smem + (ch & 1) * kPwPix * kCvRec;
    uint4 bf[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) bf[j] = *reinterpret_cast<const uint4 *>(Bs + boff[j]);
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      if (mv[i]) {
        const uint4 af = *reinterpret_cast<const uint4 *>(wa[i] + ch * wstep);
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = cv_mma<T>(af, bf[j], acc[i][j]);
      }
    }
    if (ch + 1 < NCH) stage((ch + 1) & 1);
    __syncthreads();
  }

  // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  T *ob = out + (int64_t)blockIdx.z * M * oplane;
  const T *xb = GRAD && POOL == 1 && pre_act ? x + (int64_t)blockIdx.z * M * oplane : nullptr;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (!mv[i]) continue;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int op = p0 + (wave * NB + j) * 32 + l31;                           // pixel of the low-resolution map
      if (op >= OP) continue;
      const int oy = op / Wout, ox = op - oy * Wout;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cb[i] * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= M) continue;
        float v = acc[i][j][r];
        if constexpr (GRAD && POOL == 2) {
          const T tv = (T)(v * 0.25f), zero = (T)0.f;
          T *q = ob + (int64_t)co * oplane + (int64_t)(2 * oy) * W + 2 * ox;
          q[0] = tv;
          q[1] = tv;
          q[W] = tv;
          q[W + 1] = tv;
          const bool lastx = (W & 1) && ox == Wout - 1, lasty = (H & 1) && oy == Hout - 1;   // column W - 1, row H - 1
          if (lastx) {
            q[2] = zero;
            q[W + 2] = zero;
          }
          if (lasty) {
            q[2 * (int64_t)W] = zero;
            q[2 * (int64_t)W + 1] = zero;
            if (lastx) q[2 * (int64_t)W + 2] = zero;
          }
        } else {
          const int64_t at = (int64_t)co * oplane + op;
          if constexpr (GRAD) {                          // act'(x) of the element this lane writes: x > 0 ? 1 : slope
            if (xb && !(Num<T>::ld(xb + at) > 0.f)) v *= slope;
          } else {
            if (bias) v += bias[co];
          }
          ob[at] = (T)v;
        }
      }
    }
  }
}

// launch one of the four kernels: `in` has K channels, `out` M
template <typename T>
static int pw_launch(bool grad, int pool, const T *in, const void *wp, const float *bias, const T *x, T *out, int64_t B,
                     int64_t K, int64_t M, int64_t H, int64_t W, const PwShape &s, int pre_act, float slope,
                     gfla_stream_t stream) {
  const dim3 grid((unsigned)ceil_div(s.OP, kPwPix), (unsigned)ceil_div(ceil_div(M, 32), kCvMB), (unsigned)B);
  auto launch = [&](auto p, auto g) {
    conv1x1_kernel<T, decltype(p)::value, decltype(g)::value><<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(
        in, static_cast<const unsigned char *>(wp), bias, x, out, (int)K, (int)M, (int)H, (int)W, (int)s.Hout, (int)s.Wout,
        pre_act, slope);
  };
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  if (!grad && pool == 1) launch(P1(), std::false_type());
  else if (!grad) launch(P2(), std::false_type());
  else if (pool == 1) launch(P1(), std::true_type());
  else launch(P2(), std::true_type());
  return launch_status();
}

template <typename T>
static int conv1x1_fwd(const T *x, const void *wp, const float *bias, T *y, int64_t B, int64_t Cin, int64_t Cout, int64_t H,
                       int64_t W, int pool, int pre_act, double pre_slope, gfla_stream_t stream) {
  if (!x || !wp || !y) return GFLA_ERR_NULL_POINTER;
  PwShape s;
  const int rc = pw_check(B, Cin, Cout, H, W, pool, pre_act, &s);
  if (rc != GFLA_OK) return rc;
  return pw_launch<T>(false, pool, x, wp, bias, nullptr, y, B, Cin, Cout, H, W, s, pre_act ? 1 : 0, (float)pre_slope, stream);
}

template <typename T>
static int conv1x1_bwd_data(const T *gy, const T *x, const void *wp, T *gx, int64_t B, int64_t Cin, int64_t Cout, int64_t H,
                            int64_t W, int pool, int pre_act, double pre_slope, gfla_stream_t stream) {
  if (!gy || !wp || !gx || (pre_act && !x)) return GFLA_ERR_NULL_POINTER;
  PwShape s;
  const int rc = pw_check(B, Cin, Cout, H, W, pool, pre_act, &s);
  if (rc != GFLA_OK) return rc;
  return pw_launch<T>(true, pool, gy, wp, nullptr, x, gx, B, Cout, Cin, H, W, s, pre_act ? 1 : 0, (float)pre_slope, stream);
}

static int64_t pw_packed_bytes(int64_t M, int64_t K, int elem_size) {
  if (M <= 0 || K <= 0 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (M > kCvMaxC || K > kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  return cv_packed_elems(M, K, 1, kCvRec / elem_size) * elem_size;
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_conv1x1_packed_bytes(int64_t Cout, int64_t Cin, int elem_size) {
  return gfla::pw_packed_bytes(Cout, Cin, elem_size);
}

int64_t gfla_conv1x1_grad_packed_bytes(int64_t Cout, int64_t Cin, int elem_size) {
  return gfla::pw_packed_bytes(Cin, Cout, elem_size);
}

#define GFLA_DEF_CONV1X1(SFX, T, CT)                                                                                       \
  int gfla_conv1x1_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,                \
                                      gfla_stream_t stream) {                                                              \
    return gfla::cv_pack<CT>(w, src_type, packed, Cout, Cin, 1, 0, 0, stream);                                             \
  }                                                                                                                        \
  int gfla_conv1x1_pack_grad_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,           \
                                           gfla_stream_t stream) {                                                         \
    return gfla::cv_pack<CT>(w, src_type, packed, Cin, Cout, 1, 1, 0, stream);   /* rows: x's channels */                  \
  }                                                                                                                        \
  int gfla_conv1x1_fwd_##SFX(const T *x, const void *packed, const float *bias, T *y, int64_t B, int64_t Cin,              \
                             int64_t Cout, int64_t H, int64_t W, int pool, int pre_act, double pre_slope,                  \
                             gfla_stream_t stream) {                                                                       \
    return gfla::conv1x1_fwd<CT>(reinterpret_cast<const CT *>(x), packed, bias, reinterpret_cast<CT *>(y), B, Cin, Cout,   \
                                 H, W, pool, pre_act, pre_slope, stream);                                                  \
  }                                                                                                                        \
  int gfla_conv1x1_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, int64_t B,              \
                                  int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act,                  \
                                  double pre_slope, gfla_stream_t stream) {                                                \
    return gfla::conv1x1_bwd_data<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), packed_grad,  \
                                      reinterpret_cast<CT *>(grad_x), B, Cin, Cout, H, W, pool, pre_act, pre_slope,        \
                                      stream);                                                                             \
  }
GFLA_DEF_CONV1X1(f32, float, float)
GFLA_DEF_CONV1X1(f16, uint16_t, f16_t)
GFLA_DEF_CONV1X1(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_CONV1X1
}
