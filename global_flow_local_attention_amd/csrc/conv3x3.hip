// 3x3 convolution + bias + ReLU of the VGG19 feature extractor (external_function.py:323-444), stride 1, zero padding 1,
// NCHW, as an implicit GEMM on the gfx950 matrix cores with float32 accumulation.
//
//   y[b, co, p] = max(0, bias[co] + sum over ci and the nine taps of x[b, ci, p + tap] w[co, ci, tap])
//
// GEMM view: rows = output channels, columns = pixels, reduction K = 9 Cin walked as (chunk of CK input channels) x (tap).
// One chunk fills the k of one v_mfma_f32_32x32x16_{f16,bf16} (CK = 16: lane l holds k = 8 (l >> 5) + j, sixteen bytes) or
// of four v_mfma_f32_32x32x2_f32 (CK = 8: lane l holds channels 4 (l >> 5) + q, MFMA q takes element q of both operands,
// again sixteen bytes).  In both cases a pixel of a chunk is a 32-byte record and a lane's fragment is half of it.
//
// A workgroup (4 waves) owns a TW x TH pixel tile of one sample and 64 (Cout <= 64) or 128 output channels.  Per chunk the
// (TH + 2) x (TW + 2) halo tile is staged once in LDS as [pixel][channel] records, zero outside the image and beyond Cin;
// the nine taps read it at shifted pixel offsets with ds_read_b128.  Two buffers, one barrier per chunk; the loads of the
// next chunk are in flight while the MFMAs of this one run.  The weights are the A operand, packed beforehand as
// [tap][chunk][Cout padded to 32][CK] (gfla_conv3x3_pack_weights_*), so a fragment is one 16-byte global load and a wave
// reads 2 KB contiguous; they stay in L2.  With the output channels on the MFMA rows and the pixels on the columns
// (col = lane & 31) every accumulator register holds 32 consecutive pixels of one channel plane: the NCHW store is
// coalesced.  TW is 32, 16 or 8 (narrow maps: 32 columns = 2 or 4 tile rows), whichever pads W least.
// A wave owns 2 x 2 MFMA tiles (64 channels x 64 pixels).
//
// Data gradient (the weights are frozen: no weight gradient): dX = conv3x3(g [y > 0], w mirrored, Cin <-> Cout), the same
// kernel with the ReLU mask of the saved output applied to g while it is staged; no bias, no ReLU in the epilogue.
// 16-bit outputs are rounded to nearest even once, from the float32 accumulator.  No atomics anywhere.
#include "conv_mma.h"

namespace gfla {

constexpr int kCvMB = 2;          // 32-channel MFMA tiles per wave
constexpr int kCvNB = 2;          // 32-pixel MFMA tiles per wave
constexpr int kCvItems = 11;      // 4-byte words of the halo tile a thread stages per chunk: 8 * 340 / 256 rounded up
constexpr int kCvMaxHalo = kCvItems * kBlock / 8;
constexpr int64_t kCvMaxC = 1 << 16;

// the tile a launch uses: TW = 1 << tw_log2 columns, WM waves along the output channels
struct CvTile {
  int tw_log2, WM, TH, tilesX, tilesY, halo;
};

static CvTile cv_tile(int64_t Cout, int64_t H, int64_t W) {
  CvTile g;
  g.WM = Cout > 64 ? 2 : 1;
  const int pixels = (4 / g.WM) * kCvNB * 32;
  int64_t best = -1;
  g.tw_log2 = 5;
  for (int l = 5; l >= 3; --l) {
    const int64_t padded = ceil_div(W, (int64_t)1 << l) << l;
    if (best < 0 || padded < best) {
      best = padded;
      g.tw_log2 = l;
    }
  }
  g.TH = pixels >> g.tw_log2;
  g.tilesX = (int)ceil_div(W, (int64_t)1 << g.tw_log2);
  g.tilesY = (int)ceil_div(H, g.TH);
  g.halo = (g.TH + 2) * ((1 << g.tw_log2) + 2);
  return g;
}

// x: (B, Cin, H, W), the map that is convolved (BWD: the output gradient g, Cin = its channel count); ymask (BWD): the
// saved forward output, same shape as x; wp: packed weights for Cout output channels; out: (B, Cout, H, W).
template <typename T, bool BWD>
__global__ __launch_bounds__(kBlock, 2) void conv3x3_kernel(const T *__restrict__ x, const T *__restrict__ ymask,
                                                            const unsigned char *__restrict__ wp,
                                                            const float *__restrict__ bias, T *__restrict__ out, int Cin,
                                                            int Cout, int H, int W, int tw_log2, int WM, int tilesX) {
  constexpr int CK = cv_ck<T>();
  extern __shared__ __attribute__((aligned(16))) unsigned char cv_smem[];   // [2][halo pixel][32 bytes]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
  const int WN = 4 / WM, wm = wave % WM, wn = wave / WM;
  const int TW = 1 << tw_log2, RS = 32 >> tw_log2, TH = WN * kCvNB * RS, HW = TW + 2, NPIX = HW * (TH + 2);
  const int bufB = NPIX * kCvRec;
  const int tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int y0 = tyi * TH, x0 = txi * TW;
  const int64_t plane = (int64_t)H * W;
  const T *xb = x + (int64_t)blockIdx.z * Cin * plane;
  const T *yb = BWD ? ymask + (int64_t)blockIdx.z * Cin * plane : nullptr;
  const int NCH = (Cin + CK - 1) / CK, MP = (Cout + 31) / 32 * 32;

  // what this thread stages per chunk: word q (channels 2q, 2q + 1 of the chunk, or channel q) of halo pixel p
  int goff[kCvItems], loff[kCvItems];
#pragma unroll
  for (int it = 0; it < kCvItems; ++it) {
    const int i = t + kBlock * it;
    goff[it] = loff[it] = -1;
    if (i < 8 * NPIX) {
      const int q = i / NPIX, p = i - q * NPIX, hy = p / HW, hx = p - hy * HW;
      const int gy = y0 + hy - 1, gx = x0 + hx - 1;
      loff[it] = p * kCvRec + q * 4;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) goff[it] = gy * W + gx;
    }
  }
  auto element = [&](int c, int off) -> uint32_t {
    if (c >= Cin) return 0u;
    const int64_t at = (int64_t)c * plane + off;
    if constexpr (BWD) {
      if (!(Num<T>::ld(yb + at) > 0.f)) return 0u;
    }
    return cv_bits<T>(xb + at);
  };
  uint32_t val[kCvItems];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int it = 0; it < kCvItems; ++it) {
      uint32_t v = 0u;
      if (goff[it] >= 0) {
        const int q = (loff[it] >> 2) & 7;
        if constexpr (sizeof(T) == 2) v = element(ch * CK + 2 * q, goff[it]) | (element(ch * CK + 2 * q + 1, goff[it]) << 16);
        else v = element(ch * CK + q, goff[it]);
      }
      val[it] = v;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int it = 0; it < kCvItems; ++it)
      if (loff[it] >= 0) *reinterpret_cast<uint32_t *>(cv_smem + buf * bufB + loff[it]) = val[it];
  };

  cv_f32x16 acc[kCvMB][kCvNB];
#pragma unroll
  for (int i = 0; i < kCvMB; ++i)
#pragma unroll
    for (int j = 0; j < kCvNB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // B operand: column l31 of pixel tile s = wn * NB + j is pixel (py, px) of the tile's RS rows
  const int py = l31 >> tw_log2, px = l31 & (TW - 1);
  int boff[kCvNB];
#pragma unroll
  for (int j = 0; j < kCvNB; ++j) boff[j] = (((wn * kCvNB + j) * RS + py) * HW + px) * kCvRec + kh * 16;
  // A operand: row l31 of channel tile cb; tiles beyond the padded channel count are skipped (wave-uniform)
  const int cb0 = (blockIdx.y * WM + wm) * kCvMB;
  bool mv[kCvMB];
  const unsigned char *wa[kCvMB];
#pragma unroll
  for (int i = 0; i < kCvMB; ++i) {
    mv[i] = (cb0 + i) * 32 < MP;
    wa[i] = wp + (int64_t)(mv[i] ? (cb0 + i) * 32 + l31 : 0) * kCvRec + kh * 16;
  }
  const int64_t wstep = (int64_t)MP * kCvRec;   // bytes of one (tap, chunk)

  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) fetch(ch + 1);
    const unsigned char *Bs = cv_smem + (ch & 1) * bufB;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * HW + (tap % 3)) * kCvRec;
      uint4 bf[kCvNB];
#pragma unroll
      for (int j = 0; j < kCvNB; ++j) bf[j] = *reinterpret_cast<const uint4 *>(Bs + boff[j] + toff);
#pragma unroll
      for (int i = 0; i < kCvMB; ++i) {
        if (mv[i]) {
          const uint4 af = *reinterpret_cast<const uint4 *>(wa[i] + ((int64_t)tap * NCH + ch) * wstep);
#pragma unroll
          for (int j = 0; j < kCvNB; ++j) acc[i][j] = cv_mma<T>(af, bf[j], acc[i][j]);
        }
      }
    }
    if (ch + 1 < NCH) stage((ch + 1) & 1);
    __syncthreads();
  }

  // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  T *ob = out + (int64_t)blockIdx.z * Cout * plane;
#pragma unroll
  for (int i = 0; i < kCvMB; ++i) {
    if (!mv[i]) continue;
#pragma unroll
    for (int j = 0; j < kCvNB; ++j) {
      const int gy = y0 + (wn * kCvNB + j) * RS + py, gx = x0 + px;
      if (gy >= H || gx >= W) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = (cb0 + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= Cout) continue;
        float v = acc[i][j][r];
        if constexpr (!BWD) v = fmaxf(v + bias[co], 0.f);
        ob[(int64_t)co * plane + (int64_t)gy * W + gx] = (T)v;
      }
    }
  }
}

// packed[tap][chunk][m padded to 32][CK] in T from w (Cout, Cin, 3, 3) stored as S.  layout 0 (forward): m = output
// channel, k = input channel; layout 1 (data gradient): m = input channel, k = output channel, taps mirrored.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void conv3x3_pack_kernel(const S *__restrict__ w, T *__restrict__ packed, int Cout,
                                                              int Cin, int layout, int64_t total) {
  constexpr int CK = cv_ck<T>();
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int M = layout ? Cin : Cout, K = layout ? Cout : Cin;
  const int MP = (M + 31) / 32 * 32, NCH = (K + CK - 1) / CK;
  const int j = (int)(idx % CK);
  const int m = (int)((idx / CK) % MP);
  const int ch = (int)((idx / CK / MP) % NCH);
  const int tap = (int)(idx / CK / MP / NCH);
  const int k = ch * CK + j;
  float v = 0.f;
  if (m < M && k < K) {
    const int co = layout ? k : m, ci = layout ? m : k, tp = layout ? 8 - tap : tap;
    v = Num<S>::ld(w + ((int64_t)co * Cin + ci) * 9 + tp);
  }
  packed[idx] = (T)v;
}

static int64_t cv_packed_elems(int64_t Cout, int64_t Cin, int layout, int ck) {
  const int64_t M = layout ? Cin : Cout, K = layout ? Cout : Cin;
  return 9 * ceil_div(K, ck) * (ceil_div(M, 32) * 32) * ck;
}

template <typename T>
static int conv3x3_pack(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int layout,
                        gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (Cout <= 0 || Cin <= 0 || layout < 0 || layout > 1 || src_type < 0 || src_type > 2) return GFLA_ERR_BAD_SHAPE;
  if (Cout > kCvMaxC || Cin > kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  const int64_t total = cv_packed_elems(Cout, Cin, layout, cv_ck<T>());
  const dim3 grid((unsigned)ceil_div(total, kBlock));
  hipStream_t st = static_cast<hipStream_t>(stream);
  T *dst = static_cast<T *>(packed);
  if (src_type == 0)
    conv3x3_pack_kernel<T, float><<<grid, kBlock, 0, st>>>(static_cast<const float *>(w), dst, (int)Cout, (int)Cin, layout, total);
  else if (src_type == 1)
    conv3x3_pack_kernel<T, f16_t><<<grid, kBlock, 0, st>>>(static_cast<const f16_t *>(w), dst, (int)Cout, (int)Cin, layout, total);
  else
    conv3x3_pack_kernel<T, bf16_t><<<grid, kBlock, 0, st>>>(static_cast<const bf16_t *>(w), dst, (int)Cout, (int)Cin, layout, total);
  return launch_status();
}

// Cred: channels of the convolved map, Cout: channels of the result
template <typename T, bool BWD>
static int conv3x3_launch(const T *x, const T *ymask, const void *wp, const float *bias, T *out, int64_t B, int64_t Cred,
                          int64_t Cout, int64_t H, int64_t W, gfla_stream_t stream) {
  if (B <= 0 || Cred <= 0 || Cout <= 0 || H <= 0 || W <= 0) return GFLA_ERR_BAD_SHAPE;
  if (H * W > 0x7fffffffLL || B > 65535 || Cred > kCvMaxC || Cout > kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  const CvTile g = cv_tile(Cout, H, W);
  const int64_t tiles = (int64_t)g.tilesX * g.tilesY, cblocks = ceil_div(ceil_div(Cout, 32), g.WM * kCvMB);
  if (tiles > 0x7fffffffLL || cblocks > 65535 || g.halo > kCvMaxHalo) return GFLA_ERR_UNSUPPORTED;
  const size_t lds = 2 * (size_t)g.halo * kCvRec;
  conv3x3_kernel<T, BWD><<<dim3((unsigned)tiles, (unsigned)cblocks, (unsigned)B), kBlock, lds, static_cast<hipStream_t>(stream)>>>(
      x, ymask, static_cast<const unsigned char *>(wp), bias, out, (int)Cred, (int)Cout, (int)H, (int)W, g.tw_log2, g.WM,
      g.tilesX);
  return launch_status();
}

template <typename T>
static int conv3x3_fwd(const T *x, const void *wp, const float *bias, T *y, int64_t B, int64_t Cin, int64_t Cout, int64_t H,
                       int64_t W, gfla_stream_t stream) {
  if (!x || !wp || !bias || !y) return GFLA_ERR_NULL_POINTER;
  return conv3x3_launch<T, false>(x, nullptr, wp, bias, y, B, Cin, Cout, H, W, stream);
}

template <typename T>
static int conv3x3_bwd(const T *grad_y, const T *y, const void *wp, T *grad_x, int64_t B, int64_t Cin, int64_t Cout,
                       int64_t H, int64_t W, gfla_stream_t stream) {
  if (!grad_y || !y || !wp || !grad_x) return GFLA_ERR_NULL_POINTER;
  return conv3x3_launch<T, true>(grad_y, y, wp, nullptr, grad_x, B, Cout, Cin, H, W, stream);
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_conv3x3_packed_bytes(int64_t Cout, int64_t Cin, int layout, int elem_size) {
  if (Cout <= 0 || Cin <= 0 || layout < 0 || layout > 1 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (Cout > gfla::kCvMaxC || Cin > gfla::kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  return gfla::cv_packed_elems(Cout, Cin, layout, gfla::kCvRec / elem_size) * elem_size;
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
