// The implicit-GEMM convolution family on the gfx950 matrix cores, float32 accumulation: one kernel template, one tile
// chooser, one shape check, one weight packer.  conv3x3.hip (the VGG19 extractor) and gen_conv.hip (the generators'
// bodies) hold only their entry points.
//
//   S1K3  Conv2d(k 3, s 1), one pixel of zero or reflection padding           y (B,Cout,H,W)
//   S2K4  Conv2d(k 4, s 2, p 1)                                               y (B,Cout,(H-2)/2+1,(W-2)/2+1)
//   T2K3  ConvTranspose2d(k 3, s 2, p 1, output_padding 1), w (Cin,Cout,3,3)  y (B,Cout,2H,2W)
//
// GEMM view: rows = output channels, columns = pixels of the TILED map (the output for S1K3 / S2K4, the input for T2K3),
// reduction walked as (chunk of CK input channels) x (tap).  One chunk fills the k of one v_mfma_f32_32x32x16_{f16,bf16}
// (CK = 16: lane l holds k = 8 (l >> 5) + j, sixteen bytes) or of four v_mfma_f32_32x32x2_f32 (CK = 8: lane l holds
// channels 4 (l >> 5) + q, MFMA q takes element q of both operands, again sixteen bytes).  In both cases a pixel of a
// chunk is a 32-byte record and a lane's fragment is half of it.
//
// A workgroup (4 waves) owns a TW x TH tile of the tiled map of one sample and 64 (WM = 1) or 128 (WM = 2) output
// channels; a wave owns 2 channel tiles x NB pixel tiles of 32.  Per chunk the halo tile of the input is staged once in
// LDS as [pixel][channel] records, zero outside the image and beyond Cin (S1K3 with pad_mode 1: mirrored); two buffers,
// one barrier per chunk, the loads of the next chunk in flight while the MFMAs of this one run.  The taps read the tile
// at shifted pixel offsets, one ds_read_b128 per lane.  The weights are the A operand, packed beforehand as
// [tap][chunk][Cout padded to 32][CK], so a fragment is one 16-byte global load and a wave reads 2 KB contiguous; they
// stay in L2.  With the pixels on the MFMA columns (col = lane & 31) every accumulator register holds 32 consecutive
// pixels of one channel plane: the NCHW store is coalesced.  TW is 32, 16 or 8 (narrow maps: 32 columns = 2 or 4 tile
// rows), whichever pads the tiled width least.
//
//   S1K3  halo (TH + 2) x (TW + 2); 9 taps; 256 (Cout <= 64) or 128 pixels per workgroup.
//   S2K4  halo (2 TH + 2) x (2 TW + 2); the 16 taps read records (2 py + a, 2 px + b): every lane reads its own record, the
//         stride costs nothing in LDS.  128 output pixels per workgroup (660 records = 21 KB per buffer): 256 would need 76
//         KB, beyond the 64 KB a kernel gets without opting in, and 38 staged words per thread.
//   T2K3  tiled over the INPUT, halo (TH + 1) x (TW + 1), zero at row H / column W.  Output (2i + dy, 2j + dx) is phase
//         2 dy + dx of input pixel (i, j); tap (ky, kx) belongs to phase 2 [ky != 1] + [kx != 1] and reads input pixel
//         (i + [ky == 0], j + [kx == 0]): 1 + 2 + 2 + 4 = 9 MFMA taps per pixel and chunk, never the 36 of a zero-stuffed map.
//         A wave holds the four phases of its 32 input pixels (2 channel tiles x 4 phases = 8 accumulators) and lane l31
//         stores columns 2j and 2j + 1 of an output row with one 8-byte (f32) or 4-byte (16-bit) store.
//
// What is done to an element while it is staged and to a sum before its one rounding to T is the compile-time variant:
//
//   kCvGen     y = bias + conv(act(x), w) (+ add); act = identity | LeakyReLU(slope), rounded to T once while staged;
//              bias and add may be NULL; the addend is read by the lane that writes the same element, so add == y is allowed
//   kCvVggFwd  y = max(0, bias + conv(x, w)), S1K3 only
//   kCvVggBwd  dx = conv(g [not ysaved <= 0], w), S1K3 only, the weights packed mirrored with Cin <-> Cout (the extractor is
//              frozen: no weight gradient); no bias, no ReLU
//   kCvGrad    dx = act'(x) conv(g, w) on the adjoint geometry, the weights packed for it: S1K3 mirrored with Cin <-> Cout,
//              S2K3 (the adjoint of T2K3: k 3, s 2, p 1, halo (2 TH + 1) x (2 TW + 1), the taps as stored) and U2K4 (the
//              adjoint of S2K4: tiled over the half-resolution grid, four output phases of 2 x 2 taps, halo (TH + 2) x
//              (TW + 2) of g); aux = x, act'(x) = x > 0 ? 1 : slope read by the lane that writes the element; no bias
//   kCvGradPad the S1K3 adjoint on the (H + 2) x (W + 2) padded domain of a reflect convolution, stored as float32 (the
//              fold onto x follows in gen_conv_bwd.hip)
//
// The reduction order per output element is chunk ascending, tap ascending, then the k of the MFMA.  No atomics anywhere.
#pragma once

#include <type_traits>

#include "gfla_common.h"

namespace gfla {

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 cv_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cv_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kCvRec = 32;        // bytes of one pixel (or one output channel) of one chunk
constexpr int kCvMB = 2;          // 32-channel MFMA tiles per wave
constexpr int64_t kCvMaxC = 1 << 16;
enum { kCvGen = 0, kCvVggFwd = 1, kCvVggBwd = 2, kCvGrad = 3, kCvGradPad = 4 };

// per geometry: 32-pixel MFMA tiles per wave, output phases per tiled pixel, taps, and the 4-byte words of the halo tile a
// thread stages per chunk (8 * largest halo / 256, rounded up)
struct CvGeo {
  int NB, PH, TAPS, ITEMS;
};
// 0 .. 2: the forward geometries; 3, 4: the adjoints of the two strided ones (gen_conv_bwd.hip), never an entry point's
constexpr int kCvS2K3 = 3, kCvU2K4 = 4;
constexpr CvGeo kCvGeo[5] = {{2, 1, 9, 11}, {2, 1, 16, 21}, {1, 4, 9, 6}, {2, 1, 9, 19}, {1, 4, 16, 7}};

template <typename T>
constexpr int cv_ck() { return kCvRec / (int)sizeof(T); }

template <typename T>
__device__ __forceinline__ cv_f32x16 cv_mma(uint4 a, uint4 b, cv_f32x16 acc) {
  if constexpr (__is_same(T, float)) {
    const float4 fa = __builtin_bit_cast(float4, a), fb = __builtin_bit_cast(float4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
  } else if constexpr (__is_same(T, f16_t)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cv_f16x8, a), __builtin_bit_cast(cv_f16x8, b), acc, 0,
                                                  0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cv_bf16x8, a), __builtin_bit_cast(cv_bf16x8, b), acc,
                                                   0, 0, 0);
  }
}

template <typename T>
__device__ __forceinline__ uint32_t cv_bits(const T *p) {
  if constexpr (__is_same(T, float)) return __float_as_uint(*p);
  else return p->bits;
}

// the tile a launch uses, in the coordinates of the tiled map: TW = 1 << tw_log2 columns, WM waves along the channels
struct CvTile {
  int tw_log2, WM, TH, tilesX, tilesY, halo;
  int64_t Hout, Wout;
};

static void cv_out_size(int geometry, int64_t H, int64_t W, int64_t *Hout, int64_t *Wout) {
  *Hout = geometry == 0 ? H : geometry == 1 ? (H - 2) / 2 + 1 : 2 * H;
  *Wout = geometry == 0 ? W : geometry == 1 ? (W - 2) / 2 + 1 : 2 * W;
}

// the tile of a TH_ x TW_ tiled map; Hout and Wout are the caller's to fill
static CvTile cv_tile_of(int geometry, int64_t Cout, int64_t TH_, int64_t TW_) {
  CvTile g;
  g.Hout = g.Wout = 0;
  g.WM = (geometry == 1 || geometry == kCvS2K3 || Cout > 64) ? 2 : 1;
  const int pixels = (4 / g.WM) * kCvGeo[geometry].NB * 32;
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
  g.halo = geometry == 0 || geometry == kCvU2K4 ? (g.TH + 2) * (TW + 2)
           : geometry == 1                      ? (2 * g.TH + 2) * (2 * TW + 2)
           : geometry == kCvS2K3                ? (2 * g.TH + 1) * (2 * TW + 1)
                                                : (g.TH + 1) * (TW + 1);
  return g;
}

static CvTile cv_tile(int geometry, int64_t Cout, int64_t H, int64_t W) {
  int64_t Hout, Wout;
  cv_out_size(geometry, H, W, &Hout, &Wout);
  CvTile g = cv_tile_of(geometry, Cout, geometry == 1 ? Hout : H, geometry == 1 ? Wout : W);
  g.Hout = Hout;
  g.Wout = Wout;
  return g;
}

// x: (B, Cin, H, W), the map that is convolved; wp: packed weights; bias: Cout float32 (kCvGen: or NULL; kCvVggBwd:
// unused); aux: kCvGen: the addend, y's shape, or NULL (may alias y, so neither carries __restrict__); kCvVggBwd: the saved
// forward output, x's shape; y: (B, Cout, Hout, Wout).  reflect, pre_act and slope are read by kCvGen only.
//
// WIN (the frames-major 3-D convolutions of conv3d.hip, kCvGen and kCvGrad only): x is (B, win.Lin, win.Cf, H, W) and
// blockIdx.z = b win.Lo + l counts the samples of the result.  Sample (b, l) reduces over the Cin = KT win.Cf channels of
// the KT frames that start at frame l + win.off -- contiguous in x, so the sample starts at ((b Lin + l + off) Cf) planes
// and everything else is the 2-D kernel's; channels of frames outside [0, Lin) read as zero and are never addressed.  aux
// and y are plain (B Lo, Cout, ..) batches.  A compile-time choice: without it the body is the 2-D kernel's, unchanged.
struct CvWin {
  int Lin, Lo, off, Cf;
};
struct CvNoWin {};

template <typename T, int G, int V, int WIN = 0>
__global__ __launch_bounds__(kBlock, 2) void conv_igemm_kernel(const T *__restrict__ x, const unsigned char *__restrict__ wp,
                                                               const float *__restrict__ bias, const T *aux, T *y, int Cin,
                                                               int Cout, int H, int W, int Hout, int Wout, int tw_log2,
                                                               int WM, int tilesX, int reflect, int pre_act, float slope,
                                                               std::conditional_t<WIN != 0, CvWin, CvNoWin> win = {}) {
  static_assert(!WIN || V == kCvGen || V == kCvGrad, "the window exists for the generator variant and its gradient");
  static_assert(G <= 2 || V == kCvGrad, "the adjoint geometries exist for the gradient variant only");
  static_assert(V == kCvGen || V == kCvGrad || G == 0, "the VGG variants and the padded-domain gradient exist for S1K3 only");
  static_assert(V != kCvGrad || (G != 1 && G != 2), "a gradient runs on the adjoint geometry");
  constexpr int CK = cv_ck<T>(), MB = kCvMB, NB = kCvGeo[G].NB, PH = kCvGeo[G].PH, TAPS = kCvGeo[G].TAPS;
  constexpr int ITEMS = kCvGeo[G].ITEMS;
  extern __shared__ __attribute__((aligned(16))) unsigned char cv_smem[];   // [2][halo pixel][32 bytes]

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
  const int WN = 4 / WM, wm = wave % WM, wn = wave / WM;
  const int TW = 1 << tw_log2, RS = 32 >> tw_log2, TH = WN * NB * RS;
  // halo width and height, in input pixels
  const int HW = G == 0 || G == kCvU2K4 ? TW + 2 : G == 1 ? 2 * TW + 2 : G == kCvS2K3 ? 2 * TW + 1 : TW + 1;
  const int HH = G == 0 || G == kCvU2K4 ? TH + 2 : G == 1 ? 2 * TH + 2 : G == kCvS2K3 ? 2 * TH + 1 : TH + 1;
  const int NPIX = HW * HH, bufB = NPIX * kCvRec;
  const int tyi = blockIdx.x / tilesX, txi = blockIdx.x - tyi * tilesX;
  const int y0 = tyi * TH, x0 = txi * TW;                                     // origin of the tile in the tiled map
  constexpr int O0 = V == kCvGradPad ? 2 : 1;      // kCvGradPad: the output is the padded domain, one pixel further out
  const int iy0 = G == 0 || G == kCvU2K4 ? y0 - O0 : G == 1 || G == kCvS2K3 ? 2 * y0 - 1 : y0;
  const int ix0 = G == 0 || G == kCvU2K4 ? x0 - O0 : G == 1 || G == kCvS2K3 ? 2 * x0 - 1 : x0;
  const int64_t plane = (int64_t)H * W, oplane = (int64_t)Hout * Wout;
  int clo = 0, chi = Cin;                                                     // the reduced channels that exist
  int64_t xat = (int64_t)blockIdx.z * Cin * plane;
  if constexpr (WIN) {
    const int wb = blockIdx.z / win.Lo, f0 = (int)blockIdx.z - wb * win.Lo + win.off;      // first frame of the window
    clo = f0 < 0 ? -f0 * win.Cf : 0;
    chi = win.Lin - f0 < Cin / win.Cf ? (win.Lin - f0) * win.Cf : Cin;
    xat = ((int64_t)wb * win.Lin + f0) * win.Cf * plane;
  }
  const T *xb = x + xat;
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
      if (G == 0 && V == kCvGen && reflect) {                                 // -1 -> 1, H -> H - 2 (H, W >= 2)
        gy = gy == -1 ? 1 : gy == H ? H - 2 : gy;
        gx = gx == -1 ? 1 : gx == W ? W - 2 : gx;
      }
      loff[it] = p * kCvRec + q * 4;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) goff[it] = gy * W + gx;
    }
  }
  auto element = [&](int c, int off) -> uint32_t {
    if constexpr (WIN) {
      if (c < clo || c >= chi) return 0u;
    } else {
      if (c >= Cin) return 0u;
    }
    const int64_t at = (int64_t)c * plane + off;
    if constexpr (V == kCvVggBwd) {       // the ReLU mask of the saved output; a NaN output passes its gradient on, as
      if (Num<T>::ld(aux + (xb - x) + at) <= 0.f) return 0u;                  // torch's threshold_backward does (y <= 0 ? 0 : g)
    }
    if constexpr (V == kCvGen) {
      if (pre_act) {
        const float v = Num<T>::ld(xb + at);
        const T a = (T)(v > 0.f ? v : v * slope);                             // rounded to T once, as torch hands it on
        return cv_bits<T>(&a);
      }
    }
    return cv_bits<T>(xb + at);
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
      if (loff[it] >= 0) *reinterpret_cast<uint32_t *>(cv_smem + buf * bufB + loff[it]) = val[it];
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
  constexpr int PS = G == 1 || G == kCvS2K3 ? 2 : 1;                                          // input pixels per tiled pixel
  int boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) boff[j] = (PS * ((wn * NB + j) * RS + py) * HW + PS * px) * kCvRec + kh * 16;
  // A operand: row l31 of channel tile cb[i]; tiles beyond the padded channel count are skipped (wave-uniform).  kCvGen
  // deals the tiles to the WM waves interleaved (S2K4 always has two waves along the channels: Cout = 64 keeps both busy);
  // the VGG variants (WM = 2 only beyond 64 channels) give a wave two adjacent tiles, 2 KB contiguous of packed weights:
  // the interleaved assignment measured slower over the whole extractor (three rounds of one session)
  int cb[MB];
  bool mv[MB];
  const unsigned char *wa[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    cb[i] = V == kCvVggFwd || V == kCvVggBwd ? (blockIdx.y * WM + wm) * MB + i : blockIdx.y * (WM * MB) + i * WM + wm;
    mv[i] = cb[i] * 32 < MP;
    wa[i] = wp + (int64_t)(mv[i] ? cb[i] * 32 + l31 : 0) * kCvRec + kh * 16;
  }
  const int64_t wstep = (int64_t)MP * kCvRec;   // bytes of one (tap, chunk)

  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < NCH; ++ch) {
    if (ch + 1 < NCH) fetch(ch + 1);
    const unsigned char *Bs = cv_smem + (ch & 1) * bufB;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      constexpr int KW = G == 1 || G == kCvU2K4 ? 4 : 3;
      const int ky = tap / KW, kx = tap % KW;
      // T2K3: the phase a tap feeds and the neighbour it reads; U2K4: odd taps feed the even phase (ky 1: the pixel itself,
      // ky 3: the one before), even taps the odd phase (ky 0: the one after, ky 2: itself), the halo starting one pixel
      // before the tile; the others: one phase, the tap's own offset
      const int ph = G == 2 ? 2 * (ky != 1) + (kx != 1) : G == kCvU2K4 ? 2 * !(ky & 1) + !(kx & 1) : 0;
      const int toff = (G == 2         ? (ky == 0) * HW + (kx == 0)
                        : G == kCvU2K4 ? (1 + (ky == 0) - (ky == 3)) * HW + 1 + (kx == 0) - (kx == 3)
                                       : ky * HW + kx) * kCvRec;
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
  const T *ab = (V == kCvGen || V == kCvGrad) && aux ? aux + (int64_t)blockIdx.z * Cout * oplane : nullptr;
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    if (!mv[i]) continue;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int gy = y0 + (wn * NB + j) * RS + py, gx = x0 + px;             // pixel of the tiled map
      if constexpr (G == 2) {
        if (gy >= H || gx >= W) continue;
      } else if constexpr (G == kCvU2K4) {
        if (2 * gy >= Hout || 2 * gx >= Wout) continue;
      } else {
        if (gy >= Hout || gx >= Wout) continue;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cb[i] * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (co >= Cout) continue;
        float b = 0.f;
        if constexpr (V == kCvGen) b = bias ? bias[co] : 0.f;
        if constexpr (V == kCvVggFwd) b = bias[co];
        if constexpr (G == 2) {
#pragma unroll
          for (int dy = 0; dy < 2; ++dy) {
            const int64_t at = (int64_t)co * oplane + (int64_t)(2 * gy + dy) * Wout + 2 * gx;   // even: the pair lies in one row
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
        } else if constexpr (G == kCvU2K4) {         // odd H or W: the last row / column of the odd phases does not exist
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int oy = 2 * gy + (p >> 1), ox = 2 * gx + (p & 1);
            if (oy >= Hout || ox >= Wout) continue;
            const int64_t at = (int64_t)co * oplane + (int64_t)oy * Wout + ox;
            float v = acc[i][j * PH + p][r];
            if (ab && pre_act && !(Num<T>::ld(ab + at) > 0.f)) v *= slope;
            ob[at] = (T)v;
          }
        } else {
          const int64_t at = (int64_t)co * oplane + (int64_t)gy * Wout + gx;
          float v = acc[i][j][r];
          if constexpr (V == kCvGen || V == kCvVggFwd) v += b;
          if constexpr (V == kCvVggFwd) v = v < 0.f ? 0.f : v;   // (not fmaxf: a NaN stays a NaN, as torch.relu's)
          if constexpr (V == kCvGrad) {              // act'(x) of the element this lane writes: x > 0 ? 1 : slope
            if (ab && pre_act && !(Num<T>::ld(ab + at) > 0.f)) v *= slope;
          } else {
            if (ab) v += Num<T>::ld(ab + at);
          }
          if constexpr (V == kCvGradPad) reinterpret_cast<float *>(y)[(int64_t)blockIdx.z * Cout * oplane + at] = v;
          else ob[at] = (T)v;
        }
      }
    }
  }
}

// packed[tap][chunk][m padded to 32][CK] in T from a weight stored as S with `taps` taps per channel pair: element (m, k)
// is w[m][k][tap], or with `transposed` w[k][m][tap] (ConvTranspose2d's (Cin, Cout, 3, 3); the data gradient of a Conv2d);
// with `mirror` the taps are read back to front (the data gradient)
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void conv_igemm_pack_kernel(const S *__restrict__ w, T *__restrict__ packed, int M, int K,
                                                                 int taps, int transposed, int mirror, int64_t total) {
  constexpr int CK = cv_ck<T>();
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int MP = (M + 31) / 32 * 32, NCH = (K + CK - 1) / CK;
  const int j = (int)(idx % CK);
  const int m = (int)((idx / CK) % MP);
  const int ch = (int)((idx / CK / MP) % NCH);
  const int tap = (int)(idx / CK / MP / NCH);
  const int k = ch * CK + j;
  float v = 0.f;
  if (m < M && k < K)
    v = Num<S>::ld(w + (transposed ? (int64_t)k * M + m : (int64_t)m * K + k) * taps + (mirror ? taps - 1 - tap : tap));
  packed[idx] = (T)v;
}

static int64_t cv_packed_elems(int64_t M, int64_t K, int taps, int ck) {
  return taps * ceil_div(K, ck) * (ceil_div(M, 32) * 32) * ck;
}

// M rows (the result's channels) and K reduced channels; the entry points check their own layout / geometry argument
template <typename T>
static int cv_pack(const void *w, int src_type, void *packed, int64_t M, int64_t K, int taps, int transposed, int mirror,
                   gfla_stream_t stream) {
  if (!w || !packed) return GFLA_ERR_NULL_POINTER;
  if (M <= 0 || K <= 0 || src_type < 0 || src_type > 2) return GFLA_ERR_BAD_SHAPE;
  if (M > kCvMaxC || K > kCvMaxC) return GFLA_ERR_UNSUPPORTED;
  const int64_t total = cv_packed_elems(M, K, taps, cv_ck<T>());
  auto launch = [&](auto s) {
    using S = decltype(s);
    conv_igemm_pack_kernel<T, S><<<dim3((unsigned)ceil_div(total, kBlock)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const S *>(w), static_cast<T *>(packed), (int)M, (int)K, taps, transposed, mirror, total);
  };
  if (src_type == 0) launch(float());
  else if (src_type == 1) launch(f16_t());
  else launch(bf16_t());
  return launch_status();
}

// everything that can be wrong with a shape, for the launch and for the host-only geometry query alike
static int cv_check_tile(int geometry, int64_t Cout, const CvTile &g, CvTile *tile, int64_t *cblocks);

static int cv_check(int geometry, int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pad_mode, CvTile *tile,
                    int64_t *cblocks) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || geometry < 0 || geometry > 2 || pad_mode < 0 || pad_mode > 1)
    return GFLA_ERR_BAD_SHAPE;
  if (pad_mode == 1 && (geometry != 0 || H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  if (geometry == 1 && (H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL || B > 65535 || Cin > kCvMaxC || Cout > kCvMaxC)
    return GFLA_ERR_UNSUPPORTED;
  return cv_check_tile(geometry, Cout, cv_tile(geometry, Cout, H, W), tile, cblocks);
}

// the limits of a launch with tile g (Hout and Wout filled in)
static int cv_check_tile(int geometry, int64_t Cout, const CvTile &g, CvTile *tile, int64_t *cblocks) {
  if (g.Hout * g.Wout > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  const int64_t tiles = (int64_t)g.tilesX * g.tilesY;
  *cblocks = ceil_div(ceil_div(Cout, 32), g.WM * kCvMB);
  if (tiles > 0x7fffffffLL || *cblocks > 65535 || 8 * g.halo > kCvGeo[geometry].ITEMS * kBlock) return GFLA_ERR_UNSUPPORTED;
  *tile = g;
  return GFLA_OK;
}

// check the shape, then launch variant V of the geometry (the VGG variants: geometry 0).  Pointers are the caller's to check.
template <typename T, int V>
static int cv_run(int geometry, const T *x, const void *wp, const float *bias, const T *aux, T *y, int64_t B, int64_t Cin,
                  int64_t Cout, int64_t H, int64_t W, int pad_mode, int pre_act, float slope, gfla_stream_t stream) {
  CvTile g;
  int64_t cblocks = 0;
  const int rc = cv_check(geometry, B, Cin, Cout, H, W, pad_mode, &g, &cblocks);
  if (rc != GFLA_OK) return rc;
  // T2K3 stores (and reads the addend) in pairs of elements that start at an even column: inside the map wherever y and the
  // addend lie, on a pair boundary only where they do.  Any pointer aligned to its element is taken (include/gfla_hip.h,
  // "Pointer placement")
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(aux)) % sizeof(T) != 0)
    return GFLA_ERR_UNSUPPORTED;
  auto launch = [&](auto geo) {
    conv_igemm_kernel<T, decltype(geo)::value, V>
        <<<dim3((unsigned)(g.tilesX * g.tilesY), (unsigned)cblocks, (unsigned)B), kBlock, 2 * (size_t)g.halo * kCvRec,
           static_cast<hipStream_t>(stream)>>>(x, static_cast<const unsigned char *>(wp), bias, aux, y, (int)Cin, (int)Cout,
                                               (int)H, (int)W, (int)g.Hout, (int)g.Wout, g.tw_log2, g.WM, g.tilesX, pad_mode,
                                               pre_act, slope);
  };
  if constexpr (V != kCvGen) launch(std::integral_constant<int, 0>());
  else if (geometry == 0) launch(std::integral_constant<int, 0>());
  else if (geometry == 1) launch(std::integral_constant<int, 1>());
  else launch(std::integral_constant<int, 2>());
  return launch_status();
}

}  // namespace gfla
