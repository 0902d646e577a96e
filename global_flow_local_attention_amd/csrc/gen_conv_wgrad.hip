// The weight and bias gradients of the generators' convolutions (gen_conv.hip) and of the 1x1 convolutions (conv1x1.hip) on
// the gfx950 matrix cores.
//
//   grad_w[cp][cq][tap] = sum over (b, pixel p) of P[b][cp][p] Q[b][cq][S p - 1 + tap]        float32, torch's layout
//
//   forward   P (at the reduction's pixels)   Q (tap-shifted)                  S   reduction length      grad_w
//   S1K3      g  (H x W)                      a, zero / reflect padded         1   B H W                 (Cout,Cin,3,3)
//   S2K4      g  (Hout x Wout)                a, zero padded                   2   B Hout Wout           (Cout,Cin,4,4)
//   T2K3      a  (H x W)                      g  (2H x 2W), zero outside       2   B H W                 (Cin,Cout,3,3)
//   1x1       g  (Hout x Wout)                a, or the 2 x 2 mean of x        1|2 B Hout Wout           (Cout,Cin,1,1)
//
// The 1x1 convolution of conv1x1.hip is the KW = 1 instantiation: one tap at offset 0 (Q[S p], not S p - 1 + tap), and with
// S = 2 the operand is pooled while it is staged, with the forward's expression and the forward's one rounding.
// a = act(x) is recomputed from x while it is staged, with the forward's expression (LeakyReLU rounded to T once, the
// reflect mirror): the forward saves nothing but x and the weight.
//
// GEMM view: rows = cp, columns = n = cq taps + tap (torch's flattened (cq, ky, kx)), the pixels on the k of the MFMA.  A
// workgroup (4 waves, 2 x 2) owns a 64 x 64 tile of grad_w and one range of the flattened (b, pixel) axis; a wave owns one
// 32 x 32 accumulator.  Per step of 64 pixels the workgroup stages P[64 rows][64 pixels] and the tap-shifted rows
// Q[64 columns][64 pixels] in LDS -- every column of the tile gets its own shifted copy of its row segment, so a lane's
// fragment (eight consecutive pixels of one row, 16 bytes; float32: four pixels) is one aligned ds_read_b128 whatever the
// tap, stride or mirror; rows are padded by 16 bytes against bank conflicts.  The copies cost one global (L1 / L2) read
// per element and tap; the index arithmetic per element is what bounds this kernel.
//
// The reduction is split over the pixel ranges: every workgroup writes its float32 tile into partial[split][cp][n] of an
// uninitialised workspace and a second kernel sums the splits in ascending order.  The bias gradient is one workgroup per
// channel: every thread sums its strided share of g in ascending order, then a fixed tree over the workgroup.  No atomics:
// bit-identical from call to call.
#include "conv1x1.h"
#include "conv3d.h"

namespace gfla {

constexpr int kWgTile = 64;        // rows and columns of grad_w per workgroup
constexpr int kWgPix = 64;         // pixels per step
constexpr int kWgTarget = 1024;    // workgroups a launch aims for when it chooses the number of splits
// the same for the 1x1 convolution: grad_w is one or two tiles there, so the splits are the workgroups, and the second
// kernel walks them one after the other (measured: 229 us for 1,024 splits of a 32 x 3 gradient, 0.22 us per split)
constexpr int kWgTarget1x1 = 128;

template <typename T>
__device__ __forceinline__ T wg_act(const T *p, int pre_act, float slope) {
  if (!pre_act) return *p;
  const float v = Num<T>::ld(p);
  return (T)(v > 0.f ? v : v * slope);                  // rounded to T once, as the forward stages it
}

// the mean of the 2 x 2 block at p, as conv1x1.hip's forward stages it: the float32 sum in torch's order, rounded to T once
template <typename T>
__device__ __forceinline__ T wg_pool(const T *p, int W) {
  const float s = Num<T>::ld(p) + Num<T>::ld(p + 1) + Num<T>::ld(p + W) + Num<T>::ld(p + W + 1);
  return (T)(s * 0.25f);
}

// WIN (the frames-major 3-D convolutions, conv3d.hip): P is the (B win.Lo, CP, HP, WP) batch of grad_y and Q is x
// (B, win.Lin, win.Cf, HQ, WQ); sample n = b Lo + l reads the CQ = KT Cf channels of the KT frames that start at frame
// l + win.off, channels of frames outside [0, Lin) as zero (conv_igemm.h's window).  A compile-time choice.
template <typename T, int KW, int WIN = 0>
__global__ __launch_bounds__(kBlock) void gen_conv_wgrad_kernel(const T *__restrict__ P, const T *__restrict__ Q,
                                                                float *__restrict__ partial, int CP, int CQ, int HP, int WP,
                                                                int HQ, int WQ, int S, int reflect, int act_p, int act_q,
                                                                float slope, int64_t L, int64_t per_split,
                                                                std::conditional_t<WIN != 0, CvWin, CvNoWin> win = {}) {
  static_assert(!WIN || KW == 3 || KW == 4, "the window exists for the k 3 and k 4 geometries");
  constexpr int TAPS = KW * KW, RSB = kWgPix * (int)sizeof(T) + 16, CKP = cv_ck<T>();
  __shared__ __attribute__((aligned(16))) unsigned char Ps[kWgTile * RSB];
  __shared__ __attribute__((aligned(16))) unsigned char Qs[kWgTile * RSB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, kh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int n0 = blockIdx.x * kWgTile, m0 = blockIdx.y * kWgTile, N = CQ * TAPS;
  const int col = t & 63, r0 = t >> 6;
  const int64_t planeP = (int64_t)HP * WP, planeQ = (int64_t)HQ * WQ;
  const int64_t begin = (int64_t)blockIdx.z * per_split, end = begin + per_split < L ? begin + per_split : L;

  cv_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int64_t base = begin; base < end; base += kWgPix) {
    const int64_t pix = base + col;
    const bool live = pix < end;
    const int64_t b = live ? pix / planeP : 0;
    const int rem = live ? (int)(pix - b * planeP) : 0, py = rem / WP, px = rem - py * WP;
    int clo = 0, chi = CQ;                              // the window's channels that exist, and where its sample starts
    int64_t qb = b * CQ;
    if constexpr (WIN) {
      const int64_t wb = b / win.Lo;
      const int f0 = (int)(b - wb * win.Lo) + win.off;
      clo = f0 < 0 ? -f0 * win.Cf : 0;
      chi = win.Lin - f0 < CQ / win.Cf ? (win.Lin - f0) * win.Cf : CQ;
      qb = (wb * win.Lin + f0) * win.Cf;
    }
#pragma unroll 4
    for (int i = 0; i < kWgTile / 4; ++i) {
      const int r = r0 + 4 * i, cp = m0 + r, n = n0 + r;
      T pv = (T)0.f, qv = (T)0.f;
      if (live && cp < CP) pv = wg_act<T>(P + (b * CP + cp) * planeP + rem, act_p, slope);
      if (live && n < N) {
        if constexpr (KW == 1) {                        // the pixel itself (S 1) or the mean of its 2 x 2 block (S 2)
          const T *q = Q + (b * CQ + n) * planeQ + (int64_t)(S * py) * WQ + S * px;
          qv = S == 2 ? wg_pool<T>(q, WQ) : wg_act<T>(q, act_q, slope);
        } else {
          const int cq = n / TAPS, tap = n - cq * TAPS, ky = tap / KW, kx = tap - ky * KW;
          int qy = S * py - 1 + ky, qx = S * px - 1 + kx;
          if (reflect) {                                // -1 -> 1, HQ -> HQ - 2 (HQ, WQ >= 2)
            qy = qy == -1 ? 1 : qy == HQ ? HQ - 2 : qy;
            qx = qx == -1 ? 1 : qx == WQ ? WQ - 2 : qx;
          }
          if (qy >= 0 && qy < HQ && qx >= 0 && qx < WQ && (!WIN || (cq >= clo && cq < chi)))
            qv = wg_act<T>(Q + (qb + cq) * planeQ + (int64_t)qy * WQ + qx, act_q, slope);
        }
      }
      *reinterpret_cast<T *>(Ps + r * RSB + col * (int)sizeof(T)) = pv;
      *reinterpret_cast<T *>(Qs + r * RSB + col * (int)sizeof(T)) = qv;
    }
    __syncthreads();
    // fragment k of both operands is the same pixel: 16-bit 8 kh + j of the step's sixteen, float32 4 kh + q of its eight
#pragma unroll
    for (int ks = 0; ks < kWgPix / CKP; ++ks) {
      const uint4 af = *reinterpret_cast<const uint4 *>(Ps + (32 * wm + l31) * RSB + ks * kCvRec + kh * 16);
      const uint4 bf = *reinterpret_cast<const uint4 *>(Qs + (32 * wn + l31) * RSB + ks * kCvRec + kh * 16);
      acc = cv_mma<T>(af, bf, acc);
    }
    __syncthreads();
  }

  // C/D layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float *out = partial + (int64_t)blockIdx.z * CP * N;
  const int n = n0 + 32 * wn + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cp = m0 + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (cp < CP && n < N) out[(int64_t)cp * N + n] = acc[r];
  }
}

__global__ __launch_bounds__(kBlock) void gen_conv_wgrad_reduce_kernel(const float *__restrict__ partial,
                                                                       float *__restrict__ grad_w, int splits,
                                                                       int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += partial[(int64_t)k * total + idx];
  grad_w[idx] = s;
}

// grad_b[co] = sum of g over (b, pixel): one workgroup per channel
template <typename T>
__global__ __launch_bounds__(kBlock) void gen_conv_bgrad_kernel(const T *__restrict__ g, float *__restrict__ grad_b, int C,
                                                                int64_t plane, int64_t L) {
  __shared__ float red[kBlock];
  const int co = blockIdx.x;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < L; i += kBlock) {
    const int64_t b = i / plane;
    s += Num<T>::ld(g + (b * C + co) * plane + (i - b * plane));
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad_b[co] = red[0];
}

// the launch of the weight gradient: the GEMM's sizes, the reduction length and how it is split
struct WgPlan {
  int64_t CP, CQ, HP, WP, HQ, WQ, N, L, per_split, splits, max_splits, tilesM, tilesN;
  int S, KW, act_p;
};

// the GEMM's sizes are filled in: the reduction length and how it is split
static int wg_split(WgPlan *p, int64_t target) {
  p->N = p->CQ * p->KW * p->KW;
  if (p->L > 0x7fffffffLL || p->N > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  p->tilesM = ceil_div(p->CP, kWgTile);
  p->tilesN = ceil_div(p->N, kWgTile);
  const int64_t steps = ceil_div(p->L, kWgPix), tiles = p->tilesM * p->tilesN;
  int64_t splits = target / tiles;
  splits = splits < 1 ? 1 : splits > steps ? steps : splits;
  p->max_splits = splits;                           // what the workspace is sized for: monotone in B, H and W
  p->per_split = ceil_div(steps, splits) * kWgPix;
  p->splits = ceil_div(p->L, p->per_split);
  if (p->tilesM > 65535 || p->splits > 65535) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

static int wg_plan(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, WgPlan *p) {
  CvTile fwd;
  int64_t cblocks = 0;
  const int rc = cv_check(geometry, B, Cin, Cout, H, W, pad_mode, &fwd, &cblocks);   // the forward's own limits
  if (rc != GFLA_OK) return rc;
  p->KW = geometry == 1 ? 4 : 3;
  p->S = geometry == 0 ? 1 : 2;
  p->act_p = geometry == 2;
  if (geometry == 2) {
    p->CP = Cin, p->CQ = Cout, p->HP = H, p->WP = W, p->HQ = fwd.Hout, p->WQ = fwd.Wout;
  } else {
    p->CP = Cout, p->CQ = Cin, p->HP = fwd.Hout, p->WP = fwd.Wout, p->HQ = H, p->WQ = W;
  }
  p->L = B * p->HP * p->WP;
  return wg_split(p, kWgTarget);
}

// the 1x1 convolution (conv1x1.hip): P = g at the output's pixels, Q = x at pixel `pool` p, pooled while staged (pool 2)
static int wg_plan_1x1(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act, WgPlan *p) {
  PwShape s;
  const int rc = pw_check(B, Cin, Cout, H, W, pool, pre_act, &s);                      // the forward's own limits
  if (rc != GFLA_OK) return rc;
  p->KW = 1, p->S = pool, p->act_p = 0;
  p->CP = Cout, p->CQ = Cin, p->HP = s.Hout, p->WP = s.Wout, p->HQ = H, p->WQ = W;
  p->L = B * s.OP;
  return wg_split(p, kWgTarget1x1);
}

// the launches of a plan: the split reduction and its sum, then the bias gradient over g's planes of `plane` pixels
template <typename T>
static int wg_run(const WgPlan &p, const T *gy, const T *x, float *grad_w, float *grad_b, void *ws, int64_t B, int64_t Cout,
                  int64_t plane, int pad_mode, int pre_act, double pre_slope, gfla_stream_t stream,
                  const CvWin *win = nullptr) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (grad_w) {
    const T *P = p.act_p ? x : gy, *Q = p.act_p ? gy : x;
    const int act = pre_act ? 1 : 0;
    const dim3 grid((unsigned)p.tilesN, (unsigned)p.tilesM, (unsigned)p.splits);
    auto launch = [&](auto kw) {
      if constexpr (decltype(kw)::value != 1) {
        if (win) {                                      // the frames-major 3-D convolutions: Q through the window
          gen_conv_wgrad_kernel<T, decltype(kw)::value, 1><<<grid, kBlock, 0, s>>>(
              P, Q, static_cast<float *>(ws), (int)p.CP, (int)p.CQ, (int)p.HP, (int)p.WP, (int)p.HQ, (int)p.WQ, p.S, 0, 0, act,
              (float)pre_slope, p.L, p.per_split, *win);
          return;
        }
      }
      gen_conv_wgrad_kernel<T, decltype(kw)::value><<<grid, kBlock, 0, s>>>(
          P, Q, static_cast<float *>(ws), (int)p.CP, (int)p.CQ, (int)p.HP, (int)p.WP, (int)p.HQ, (int)p.WQ, p.S, pad_mode,
          p.act_p ? act : 0, p.act_p ? 0 : act, (float)pre_slope, p.L, p.per_split);
    };
    if (p.KW == 4) launch(std::integral_constant<int, 4>());
    else if (p.KW == 3) launch(std::integral_constant<int, 3>());
    else launch(std::integral_constant<int, 1>());
    int st = launch_status();
    if (st != GFLA_OK) return st;
    const int64_t total = p.CP * p.N;
    gen_conv_wgrad_reduce_kernel<<<dim3((unsigned)ceil_div(total, kBlock)), kBlock, 0, s>>>(
        static_cast<const float *>(ws), grad_w, (int)p.splits, total);
    st = launch_status();
    if (st != GFLA_OK) return st;
  }
  if (grad_b) gen_conv_bgrad_kernel<T><<<dim3((unsigned)Cout), kBlock, 0, s>>>(gy, grad_b, (int)Cout, plane, B * plane);
  return launch_status();
}

template <typename T>
static int gen_conv_bwd_weight(const T *gy, const T *x, float *grad_w, float *grad_b, void *ws, int64_t B, int64_t Cin,
                               int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, int pre_act, double pre_slope,
                               gfla_stream_t stream) {
  if (!gy || (!grad_w && !grad_b) || (grad_w && (!x || !ws))) return GFLA_ERR_NULL_POINTER;
  WgPlan p;
  const int rc = wg_plan(B, Cin, Cout, H, W, geometry, pad_mode, &p);
  if (rc != GFLA_OK) return rc;
  const CvTile fwd = cv_tile(geometry, Cout, H, W);
  return wg_run<T>(p, gy, x, grad_w, grad_b, ws, B, Cout, fwd.Hout * fwd.Wout, pad_mode, pre_act, pre_slope, stream);
}

template <typename T>
static int conv1x1_bwd_weight(const T *gy, const T *x, float *grad_w, float *grad_b, void *ws, int64_t B, int64_t Cin,
                              int64_t Cout, int64_t H, int64_t W, int pool, int pre_act, double pre_slope,
                              gfla_stream_t stream) {
  if (!gy || (!grad_w && !grad_b) || (grad_w && (!x || !ws))) return GFLA_ERR_NULL_POINTER;
  WgPlan p;
  const int rc = wg_plan_1x1(B, Cin, Cout, H, W, pool, pre_act, &p);
  if (rc != GFLA_OK) return rc;
  return wg_run<T>(p, gy, x, grad_w, grad_b, ws, B, Cout, p.HP * p.WP, 0, pre_act, pre_slope, stream);
}

// the frames-major 3-D convolutions (conv3d.hip): P = g, a (B Lout, Cout, Hout, Wout) batch; Q = x through the window
static int wg_plan_3d(int64_t B, int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, WgPlan *p,
                      C3Shape *s) {
  const int rc = c3_check(B, L, C, Cout, H, W, geometry, s);                            // the forward's own limits
  if (rc != GFLA_OK) return rc;
  p->KW = geometry == 1 ? 4 : 3;
  p->S = geometry == 0 ? 1 : 2;
  p->act_p = 0;
  p->CP = Cout, p->CQ = kC3KT * C, p->HP = s->Hout, p->WP = s->Wout, p->HQ = H, p->WQ = W;
  p->L = B * s->Lout * s->Hout * s->Wout;
  return wg_split(p, kWgTarget);
}

template <typename T>
static int conv3d_bwd_weight(const T *gy, const T *x, float *grad_w, float *grad_b, void *ws, int64_t B, int64_t L,
                             int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act, double pre_slope,
                             gfla_stream_t stream) {
  if (!gy || (!grad_w && !grad_b) || (grad_w && (!x || !ws))) return GFLA_ERR_NULL_POINTER;
  WgPlan p;
  C3Shape s;
  const int rc = wg_plan_3d(B, L, C, Cout, H, W, geometry, &p, &s);
  if (rc != GFLA_OK) return rc;
  const CvWin win = {(int)L, (int)s.Lout, -s.pt, (int)C};
  return wg_run<T>(p, gy, x, grad_w, grad_b, ws, B * s.Lout, Cout, s.Hout * s.Wout, 0, pre_act, pre_slope, stream, &win);
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_gen_conv_bwd_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry,
                                          int pad_mode, int elem_size) {
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  gfla::WgPlan p;
  const int rc = gfla::wg_plan(B, Cin, Cout, H, W, geometry, pad_mode, &p);
  if (rc != GFLA_OK) return rc;
  if (pad_mode == 1 && (H + 2) * (W + 2) > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;       // what bwd_data refuses
  const int64_t weight = p.max_splits * p.CP * p.N * 4;                                  // the float32 partial sums
  const int64_t data = pad_mode == 1 ? B * Cin * (H + 2) * (W + 2) * 4 : 0;          // grad_p of the reflect case
  return (weight > data ? weight : data) + 16;
}

int64_t gfla_conv1x1_bwd_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool,
                                         int elem_size) {
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  gfla::WgPlan p;
  const int rc = gfla::wg_plan_1x1(B, Cin, Cout, H, W, pool, 0, &p);
  if (rc != GFLA_OK) return rc;
  return p.max_splits * p.CP * p.N * 4 + 16;                                             // the float32 partial sums
}

int64_t gfla_conv3d_bwd_workspace_bytes(int64_t B, int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry,
                                        int elem_size) {
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  gfla::WgPlan p;
  gfla::C3Shape s;
  const int rc = gfla::wg_plan_3d(B, L, C, Cout, H, W, geometry, &p, &s);
  if (rc != GFLA_OK) return rc;
  return p.max_splits * p.CP * p.N * 4 + 16;                                             // the float32 partial sums
}

#define GFLA_DEF_GEN_CONV_WGRAD(SFX, T, CT)                                                                               \
  int gfla_gen_conv_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace,          \
                                     int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry,            \
                                     int pad_mode, int pre_act, double pre_slope, gfla_stream_t stream) {                 \
    return gfla::gen_conv_bwd_weight<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), grad_w,   \
                                         grad_b, workspace, B, Cin, Cout, H, W, geometry, pad_mode, pre_act, pre_slope,   \
                                         stream);                                                                         \
  }                                                                                                                       \
  int gfla_conv1x1_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace,           \
                                    int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act,    \
                                    double pre_slope, gfla_stream_t stream) {                                             \
    return gfla::conv1x1_bwd_weight<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), grad_w,    \
                                        grad_b, workspace, B, Cin, Cout, H, W, pool, pre_act, pre_slope, stream);         \
  }
#define GFLA_DEF_CONV3D_WGRAD(SFX, T, CT)                                                                                 \
  int gfla_conv3d_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace, int64_t B, \
                                   int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act,   \
                                   double pre_slope, gfla_stream_t stream) {                                              \
    return gfla::conv3d_bwd_weight<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<const CT *>(x), grad_w,     \
                                       grad_b, workspace, B, L, C, Cout, H, W, geometry, pre_act, pre_slope, stream);     \
  }
GFLA_DEF_CONV3D_WGRAD(f32, float, float)
GFLA_DEF_CONV3D_WGRAD(f16, uint16_t, f16_t)
GFLA_DEF_CONV3D_WGRAD(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_CONV3D_WGRAD
GFLA_DEF_GEN_CONV_WGRAD(f32, float, float)
GFLA_DEF_GEN_CONV_WGRAD(f16, uint16_t, f16_t)
GFLA_DEF_GEN_CONV_WGRAD(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_GEN_CONV_WGRAD
}
