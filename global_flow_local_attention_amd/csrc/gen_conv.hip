// The convolutions of the generators' bodies (base_function.py:334-391 EncoderBlock / ResBlock, 508-531 ResBlockDecoder,
// 672-691 Jump), forward only, frozen weights, as implicit GEMMs on the gfx950 matrix cores with float32 accumulation:
//
//   S1K3  Conv2d(k 3, s 1), one pixel of zero or reflection padding           y (B,Cout,H,W)
//   S2K4  Conv2d(k 4, s 2, p 1)                                               y (B,Cout,(H-2)/2+1,(W-2)/2+1)
//   T2K3  ConvTranspose2d(k 3, s 2, p 1, output_padding 1), w (Cin,Cout,3,3)  y (B,Cout,2H,2W)
//
//   y = bias + conv(act(x), w) (+ add),   act = identity | LeakyReLU(pre_slope), rounded to T once while it is staged
//
// One template in the style of conv3x3_kernel (conv3x3.hip), three geometries.  GEMM view: rows = output channels, columns
// = pixels of the TILED map (the output for S1K3 / S2K4, the input for T2K3), reduction walked as (chunk of CK input
// channels) x (tap).  Per chunk the halo tile of the input is staged once in LDS as 32-byte [pixel][channel-chunk] records,
// zero outside the image and beyond Cin (S1K3 with pad_mode 1: mirrored); two buffers, one barrier per chunk, the loads of
// the next chunk in flight while the MFMAs of this one run.  The taps read the tile at shifted pixel offsets, one 16-byte
// LDS load per lane.  A fragments are single 16-byte loads from the packed weights [tap][chunk][Cout padded to 32][CK].
//
//   S1K3  halo (TH + 2) x (TW + 2); 9 taps; a wave owns 2 x 2 MFMA tiles; 256 or 128 pixels per workgroup as in conv3x3.
//   S2K4  halo (2 TH + 2) x (2 TW + 2); the 16 taps read records (2 py + a, 2 px + b): every lane reads its own record, the
//         stride costs nothing in LDS.  128 output pixels per workgroup (660 records = 21 KB per buffer): 256 would need 76
//         KB, beyond the 64 KB a kernel gets without opting in, and 38 staged words per thread.
//   T2K3  tiled over the INPUT, halo (TH + 1) x (TW + 1), zero at row H / column W.  Output (2i + dy, 2j + dx) is phase
//         2 dy + dx of input pixel (i, j); tap (ky, kx) belongs to phase 2 [ky != 1] + [kx != 1] and reads input pixel
//         (i + [ky == 0], j + [kx == 0]): 1 + 2 + 2 + 4 = 9 MFMA taps per pixel and chunk, never the 36 of a zero-stuffed map.
//         A wave holds the four phases of its 32 input pixels (2 channel tiles x 4 phases = 8 accumulators) and lane l31
//         stores columns 2j and 2j + 1 of an output row with one 8-byte (f32) or 4-byte (16-bit) store.
//
// Epilogue: bias (float32, or none) and the optional addend (y's shape and type) are added in float32, then one rounding.
// The addend is read by the lane that writes the same element, so add == y is allowed.  No atomics.
#include "conv_mma.h"

namespace gfla {

constexpr int64_t kGcMaxC = 1 << 16;

template <int G>
struct GcGeo;
template <>
struct GcGeo<0> {   // S1K3
  static constexpr int MB = 2, NB = 2, PH = 1, TAPS = 9, ITEMS = 11;
};
template <>
struct GcGeo<1> {   // S2K4
  static constexpr int MB = 2, NB = 2, PH = 1, TAPS = 16, ITEMS = 21;
};
template <>
struct GcGeo<2> {   // T2K3
  static constexpr int MB = 2, NB = 1, PH = 4, TAPS = 9, ITEMS = 6;
};

static int gc_taps(int geometry) { return geometry == 1 ? 16 : 9; }
static int gc_items(int geometry) { return geometry == 0 ? GcGeo<0>::ITEMS : geometry == 1 ? GcGeo<1>::ITEMS : GcGeo<2>::ITEMS; }
static int gc_nb(int geometry) { return geometry == 2 ? 1 : 2; }

// the tile a launch uses, in the coordinates of the tiled map: TW = 1 << tw_log2 columns, WM waves along the channels
struct GcTile {
  int tw_log2, WM, TH, tilesX, tilesY, halo;
  int64_t Hout, Wout;
};

static void gc_out_size(int geometry, int64_t H, int64_t W, int64_t *Hout, int64_t *Wout) {
  *Hout = geometry == 0 ? H : geometry == 1 ? (H - 2) / 2 + 1 : 2 * H;
  *Wout = geometry == 0 ? W : geometry == 1 ? (W - 2) / 2 + 1 : 2 * W;
}

static GcTile gc_tile(int geometry, int64_t Cout, int64_t H, int64_t W) {
  GcTile g;
  gc_out_size(geometry, H, W, &g.Hout, &g.Wout);
  const int64_t TH_ = geometry == 1 ? g.Hout : H, TW_ = geometry == 1 ? g.Wout : W;    // the tiled map
  g.WM = (geometry == 1 || Cout > 64) ? 2 : 1;
  const int pixels = (4 / g.WM) * gc_nb(geometry) * 32;
  int64_t best = -1;
  g.tw_log2 = 5;
  for (int l = 5; l >= 3; --l) {
    const int64_t padded = ceil_div(TW_, (int64_t)1 << l) << l;
    if (best < 0 || padded < best) {
      best = padded;
      g.tw_log2 = l;
    }
  }
  const int TW = 1 << g.tw_log2;
  g.TH = pixels >> g.tw_log2;
  g.tilesX = (int)ceil_div(TW_, TW);
  g.tilesY = (int)ceil_div(TH_, g.TH);
  g.halo = geometry == 0 ? (g.TH + 2) * (TW + 2) : geometry == 1 ? (2 * g.TH + 2) * (2 * TW + 2) : (g.TH + 1) * (TW + 1);
  return g;
}

// x: (B, Cin, H, W); wp: packed weights; bias: Cout float32 or NULL; add: y's shape or NULL (may alias y); y: (B, Cout,
// Hout, Wout).  add and y carry no __restrict__: they may be the same tensor.
template <typename T, int G>
__global__ __launch_bounds__(kBlock, 2) void gen_conv_kernel(const T *__restrict__ x, const unsigned char *__restrict__ wp,
                                                             const float *__restrict__ bias, const T *add, T *y, int Cin,
                                                             int Cout, int H, int W, int Hout, int Wout, int tw_log2, int WM,
                                                             int tilesX, int reflect, int pre_act, float slope) {
  using Geo = GcGeo<G>;
  constexpr int CK = cv_ck<T>(), MB = Geo::MB, NB = Geo::NB, PH = Geo::PH, TAPS = Geo::TAPS, ITEMS = Geo::ITEMS;
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_smem[];   // [2][halo pixel][32 bytes]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
  const int WN = 4 / WM, wm = wave % WM, wn = wave / WM;
  const int TW = 1 << tw_log2, RS = 32 >> tw_log2, TH = WN * NB * RS;
  const int HW = G == 0 ? TW + 2 : G == 1 ? 2 * TW + 2 : TW + 1;              // halo width and height, in input pixels
  const int HH = G == 0 ? TH + 2 : G == 1 ? 2 * TH + 2 : TH + 1;
  const int NPIX = HW * HH, bufB = NPIX * kCvRec;
  const int tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int y0 = tyi * TH, x0 = txi * TW;                                     // origin of the tile in the tiled map
  const int iy0 = G == 0 ? y0 - 1 : G == 1 ? 2 * y0 - 1 : y0, ix0 = G == 0 ? x0 - 1 : G == 1 ? 2 * x0 - 1 : x0;
  const int64_t plane = (int64_t)H * W, oplane = (int64_t)Hout * Wout;
  const T *xb = x + (int64_t)blockIdx.z * Cin * plane;
  const int NCH = (Cin + CK - 1) / CK, MP = (Cout + 31) / 32 * 32;

  // what this thread stages per chunk: word q (channels 2q, 2q + 1 of the chunk, or channel q) of halo pixel p
  int goff[ITEMS], loff[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int i = t + kBlock * it;
    goff[it] = loff[it] = -1;
    if (i < 8 * NPIX) {
      const int q = i / NPIX, p = i - q * NPIX, hy = p / HW, hx = p - hy * HW;
      int gy = iy0 + hy, gx = ix0 + hx;
      if (G == 0 && reflect) {                                                // -1 -> 1, H -> H - 2 (H, W >= 2)
        gy = gy == -1 ? 1 : gy == H ? H - 2 : gy;
        gx = gx == -1 ? 1 : gx == W ? W - 2 : gx;
      }
      loff[it] = p * kCvRec + q * 4;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) goff[it] = gy * W + gx;
    }
  }
  auto element = [&](int c, int off) -> uint32_t {
    if (c >= Cin) return 0u;
    const T *p = xb + (int64_t)c * plane + off;
    if (pre_act) {
      const float v = Num<T>::ld(p);
      const T a = (T)(v > 0.f ? v : v * slope);                               // rounded to T once, as torch hands it on
      return cv_bits<T>(&a);
    }
    return cv_bits<T>(p);
  };
  uint32_t val[ITEMS];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
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
    for (int it = 0; it < ITEMS; ++it)
      if (loff[it] >= 0) *reinterpret_cast<uint32_t *>(gc_smem + buf * bufB + loff[it]) = val[it];
  };

  cv_f32x16 acc[MB][NB * PH];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int j = 0; j < NB * PH; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // B operand: column l31 of pixel tile s = wn * NB + j is pixel (py, px) of the tile's RS rows
  const int py = l31 >> tw_log2, px = l31 & (TW - 1);
  constexpr int PS = G == 1 ? 2 : 1;                                          // input pixels per tiled pixel
  int boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) boff[j] = (PS * ((wn * NB + j) * RS + py) * HW + PS * px) * kCvRec + kh * 16;
  // A operand: row l31 of channel tile cb[i], interleaved over the waves; tiles beyond the padded channel count are
  // skipped (wave-uniform)
  int cb[MB];
  bool mv[MB];
  const unsigned char *wa[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    cb[i] = blockIdx.y * (WM * MB) + i * WM + wm;
    mv[i] = cb[i] * 32 < MP;
    wa[i] = wp + (int64_t)(mv[i] ? cb[i] * 32 + l31 : 0) * kCvRec + kh * 16;
  }
  const int64_t wstep = (int64_t)MP * kCvRec;   // bytes of one (tap, chunk)

  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) fetch(ch + 1);
    const unsigned char *Bs = gc_smem + (ch & 1) * bufB;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      constexpr int KW = G == 1 ? 4 : 3;
      const int ky = tap / KW, kx = tap % KW;
      // T2K3: the phase a tap feeds and the neighbour it reads; the others: one phase, the tap's own offset
      const int ph = G == 2 ? 2 * (ky != 1) + (kx != 1) : 0;
      const int toff = (G == 2 ? (ky == 0) * HW + (kx == 0) : ky * HW + kx) * kCvRec;
      uint4 bf[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) bf[j] = *reinterpret_cast<const uint4 *>(Bs + boff[j] + toff);
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        if (mv[i]) {
          const uint4 af = *reinterpret_cast<const uint4 *>(wa[i] + ((int64_t)tap * NCH + ch) * wstep);
#pragma unroll
          for (int j = 0; j < NB; ++j) acc[i][j * PH + ph] = cv_mma<T>(af, bf[j], acc[i][j * PH + ph]);
        }
      }
    }
    if (ch + 1 < NCH) stage((ch + 1) & 1);
    __syncthreads();
  }

  // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  T *ob = y + (int64_t)blockIdx.z * Cout * oplane;
  const T *ab = add ? add + (int64_t)blockIdx.z * Cout * oplane : nullptr;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (!mv[i]) continue;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int gy = y0 + (wn * NB + j) * RS + py, gx = x0 + px;             // pixel of the tiled map
      if constexpr (G == 2) {
        if (gy >= H || gx >= W) continue;
      } else {
        if (gy >= Hout || gx >= Wout) continue;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cb[i] * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= Cout) continue;
        const float b = bias ? bias[co] : 0.f;
        if constexpr (G == 2) {
#pragma unroll
          for (int dy = 0; dy < 2; ++dy) {
            const int64_t at = (int64_t)co * oplane + (int64_t)(2 * gy + dy) * Wout + 2 * gx;   // even: the pair is aligned
            float v0 = acc[i][j * PH + 2 * dy][r] + b, v1 = acc[i][j * PH + 2 * dy + 1][r] + b;
            if (ab) {
              const Pack<T, 2> a = *reinterpret_cast<const Pack<T, 2> *>(ab + at);
              v0 += Num<T>::ld(&a.v[0]);
              v1 += Num<T>::ld(&a.v[1]);
            }
            Pack<T, 2> o;
            o.v[0] = (T)v0;
            o.v[1] = (T)v1;
            *reinterpret_cast<Pack<T, 2> *>(ob + at) = o;
          }
        } else {
          const int64_t at = (int64_t)co * oplane + (int64_t)gy * Wout + gx;
          float v = acc[i][j][r] + b;
          if (ab) v += Num<T>::ld(ab + at);
          ob[at] = (T)v;
        }
      }
    }
  }
}

// packed[tap][chunk][co padded to 32][CK] in T from torch's weight as stored (S): (Cout, Cin, k, k) of a Conv2d (geometry 0,
// 1), (Cin, Cout, 3, 3) of a ConvTranspose2d (geometry 2); tap = ky k + kx.
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void gen_conv_pack_kernel(const S *__restrict__ w, T *__restrict__ packed, int Cout,
                                                               int Cin, int geometry, int64_t total) {
  constexpr int CK = cv_ck<T>();
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int taps = geometry == 1 ? 16 : 9;
  const int MP = (Cout + 31) / 32 * 32, NCH = (Cin + CK - 1) / CK;
  const int j = (int)(idx % CK);
  const int m = (int)((idx / CK) % MP);
  const int ch = (int)((idx / CK / MP) % NCH);
  const int tap = (int)(idx / CK / MP / NCH);
  const int k = ch * CK + j;
  float v = 0.f;
  if (m < Cout && k < Cin)
    v = Num<S>::ld(w + (geometry == 2 ? (int64_t)k * Cout + m : (int64_t)m * Cin + k) * taps + tap);
  packed[idx] = (T)v;
}

static int64_t gc_packed_elems(int64_t Cout, int64_t Cin, int geometry, int ck) {
  return gc_taps(geometry) * ceil_div(Cin, ck) * (ceil_div(Cout, 32) * 32) * ck;
}

template <typename T>
static int gen_conv_pack(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int geometry,
                         gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (Cout <= 0 || Cin <= 0 || geometry < 0 || geometry > 2 || src_type < 0 || src_type > 2) return GFLA_ERR_BAD_SHAPE;
  if (Cout > kGcMaxC || Cin > kGcMaxC) return GFLA_ERR_UNSUPPORTED;
  const int64_t total = gc_packed_elems(Cout, Cin, geometry, cv_ck<T>());
  const dim3 grid((unsigned)ceil_div(total, kBlock));
  hipStream_t st = static_cast<hipStream_t>(stream);
  T *dst = static_cast<T *>(packed);
  if (src_type == 0)
    gen_conv_pack_kernel<T, float><<<grid, kBlock, 0, st>>>(static_cast<const float *>(w), dst, (int)Cout, (int)Cin, geometry, total);
  else if (src_type == 1)
    gen_conv_pack_kernel<T, f16_t><<<grid, kBlock, 0, st>>>(static_cast<const f16_t *>(w), dst, (int)Cout, (int)Cin, geometry, total);
  else
    gen_conv_pack_kernel<T, bf16_t><<<grid, kBlock, 0, st>>>(static_cast<const bf16_t *>(w), dst, (int)Cout, (int)Cin, geometry, total);
  return launch_status();
}

// everything that can be wrong with a shape, for the launch and for the host-only geometry query alike
static int gc_check(int geometry, int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pad_mode, GcTile *tile,
                    int64_t *cblocks) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || geometry < 0 || geometry > 2 || pad_mode < 0 || pad_mode > 1)
    return GFLA_ERR_BAD_SHAPE;
  if (pad_mode == 1 && (geometry != 0 || H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  if (geometry == 1 && (H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL || B > 65535 || Cin > kGcMaxC || Cout > kGcMaxC)
    return GFLA_ERR_UNSUPPORTED;
  const GcTile g = gc_tile(geometry, Cout, H, W);
  if (g.Hout * g.Wout > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  const int64_t tiles = (int64_t)g.tilesX * g.tilesY;
  *cblocks = ceil_div(ceil_div(Cout, 32), g.WM * 2);
  if (tiles > 0x7fffffffLL || *cblocks > 65535 || 8 * g.halo > gc_items(geometry) * kBlock) return GFLA_ERR_UNSUPPORTED;
  *tile = g;
  return GFLA_OK;
}

template <typename T, int G>
static int gen_conv_launch(const T *x, const void *wp, const float *bias, const T *add, T *y, int64_t B, int64_t Cin,
                           int64_t Cout, int64_t H, int64_t W, const GcTile &g, int64_t cblocks, int pad_mode, int pre_act,
                           float slope, gfla_stream_t stream) {
  static_assert(GcGeo<G>::MB == 2, "gc_check counts two channel tiles per wave");
  const size_t lds = 2 * (size_t)g.halo * kCvRec;
  gen_conv_kernel<T, G><<<dim3((unsigned)(g.tilesX * g.tilesY), (unsigned)cblocks, (unsigned)B), kBlock, lds,
                          static_cast<hipStream_t>(stream)>>>(x, static_cast<const unsigned char *>(wp), bias, add, y, (int)Cin,
                                                              (int)Cout, (int)H, (int)W, (int)g.Hout, (int)g.Wout, g.tw_log2,
                                                              g.WM, g.tilesX, pad_mode, pre_act, slope);
  return launch_status();
}

template <typename T>
static int gen_conv_fwd(const T *x, const void *wp, const float *bias, const T *add, T *y, int64_t B, int64_t Cin,
                        int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, int pre_act, double pre_slope,
                        gfla_stream_t stream) {
  if (!x || !wp || !y) return GFLA_ERR_NULL_POINTER;
  GcTile g;
  int64_t cblocks = 0;
  const int rc = gc_check(geometry, B, Cin, Cout, H, W, pad_mode, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  // T2K3 stores (and reads the addend) in pairs of elements
  if (geometry == 2 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(add)) % (2 * sizeof(T))) != 0)
    return GFLA_ERR_UNSUPPORTED;
  const float slope = (float)pre_slope;
  const int act = pre_act ? 1 : 0;
  if (geometry == 0) return gen_conv_launch<T, 0>(x, wp, bias, add, y, B, Cin, Cout, H, W, g, cblocks, pad_mode, act, slope, stream);
  if (geometry == 1) return gen_conv_launch<T, 1>(x, wp, bias, add, y, B, Cin, Cout, H, W, g, cblocks, 0, act, slope, stream);
  return gen_conv_launch<T, 2>(x, wp, bias, add, y, B, Cin, Cout, H, W, g, cblocks, 0, act, slope, stream);
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_gen_conv_packed_bytes(int64_t Cout, int64_t Cin, int geometry, int elem_size) {
  if (Cout <= 0 || Cin <= 0 || geometry < 0 || geometry > 2 || (elem_size != 2 && elem_size != 4)) return GFLA_ERR_BAD_SHAPE;
  if (Cout > gfla::kGcMaxC || Cin > gfla::kGcMaxC) return GFLA_ERR_UNSUPPORTED;
  return gfla::gc_packed_elems(Cout, Cin, geometry, gfla::kCvRec / elem_size) * elem_size;
}

int gfla_gen_conv_out_size(int geometry, int64_t H, int64_t W, int64_t *Hout, int64_t *Wout) {
  if (!Hout || !Wout) return GFLA_ERR_NULL_POINTER;
  if (geometry < 0 || geometry > 2 || H <= 0 || W <= 0 || (geometry == 1 && (H < 2 || W < 2))) return GFLA_ERR_BAD_SHAPE;
  gfla::gc_out_size(geometry, H, W, Hout, Wout);
  return GFLA_OK;
}

int gfla_gen_conv_geometry(int geometry, int64_t Cout, int64_t H, int64_t W, int elem_size, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  gfla::GcTile g;
  int64_t cblocks = 0;
  const int rc = gfla::gc_check(geometry, 1, 1, Cout, H, W, 0, &g, &cblocks);
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
