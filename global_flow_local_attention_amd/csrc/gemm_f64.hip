// Float64 GEMM on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), gfx950: the two FC layers of ExtractorAttn in
// float64 (global_flow_local_attention_amd/fc_f64.py).
//
//   C[m,n] = beta*C[m,n] + sum_k A[m,k] * B[k,n],   beta in {0, 1}
//
// Every operand is a VIEW: each of its two logical indices x is split into up to three sub-indices
// x = (x0*d1 + x1)*d2 + x2, each with its own element stride.  So the kernel reads and writes in place the conv0 weight
// (128, 2C*k*k) and either half of it, the extractor's unfold layout (C*k*k, B, H, W), the reference block layout
// (B, C, H*k, W*k) with K = (c, i, j) and N = (b, h, w), the (B, 128, H, W) hidden maps and their transposes -- no
// packed copies, no transposes in HBM.
//
// Tiling: a 256-thread workgroup computes a 128 x 64 tile of C (the 128 hidden channels of the FC layer in one tile, so
// the large operand is read once), each wave a 64 x 32 quarter as 4 x 2 MFMA blocks.  K advances by 16: the next
// K-slab is fetched into registers while the current one is multiplied out of LDS.  Both LDS slabs are k-major
// ([k][m] and [k][n]): an MFMA operand fragment is then 16 consecutive doubles per k row.
//
// Long reductions (the weight gradients: K = B*H*W) use a deterministic split-K: slice z of K writes its partial tile
// to workspace[z][M][N], and a second pass sums the slices in order z = 0, 1, ... and applies beta.  No float atomics:
// identical inputs give bit-identical results.
//
// f64 MFMA accumulator layout (NOT the f32 one): result register r of lane l holds C[row (l>>4) + 4r][col l&15] of the
// 16 x 16 block; A and B fragments are one double per lane, A[row l&15][k l>>4] and B[k l>>4][col l&15].
#include "gfla_common.h"

#include <algorithm>

namespace gfla {
namespace {

constexpr int kGM = 128, kGN = 64, kGK = 16, kGThreads = 256;
constexpr int kPitchA = kGM + 16, kPitchB = kGN + 16;  // LDS row pitch in doubles: k rows alternate 128-byte bank halves
constexpr int kLoadA = kGM * kGK / kGThreads;          // 8 elements of A per thread per K-slab
constexpr int kLoadB = kGK * kGN / kGThreads;          // 4 elements of B

using f64x4 = __attribute__((ext_vector_type(4))) double;

// One logical index of an operand: x = (x0*d1 + x1)*d2 + x2, element offset x0*s0 + x1*s1 + x2*s2.
struct Axis {
  uint32_t d1, d2;
  int64_t s0, s1, s2;
  __device__ __forceinline__ int64_t off(uint32_t x) const {
    if (d1 == 1 && d2 == 1) return (int64_t)x * s0;  // (wave-uniform) plain strided index
    const uint32_t q = x / d2, x2 = x - q * d2;
    const uint32_t x0 = q / d1, x1 = q - x0 * d1;
    return (int64_t)x0 * s0 + (int64_t)x1 * s1 + (int64_t)x2 * s2;
  }
};

struct View {
  Axis r, c;   // element (row, col) at base + r.off(row) + c.off(col)
  bool c_fast;  // the column index has the smaller innermost stride: consecutive threads walk columns when loading
};

struct GemmArgs {
  double *c;
  const double *a, *b;
  View cv, av, bv;
  int M, N, K, beta;
  int k_slice;     // K per split-K slice (a multiple of kGK); one slice = the whole K
  double *part;    // split-K: [slices][M][N] partial products; NULL = write C directly
};

__global__ __launch_bounds__(kGThreads) void gemm_f64_kernel(const GemmArgs g) {
  __shared__ double As[kGK][kPitchA];
  __shared__ double Bs[kGK][kPitchB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * kGM, n0 = blockIdx.x * kGN;
  const int kbeg = blockIdx.z * g.k_slice, kend = min(g.K, kbeg + g.k_slice);

  // Loader geometry.  A tile (128 x 16): k-fast -> kk = t&15 (fixed), mm = (t>>4) + 16i; else mm = t&127, kk = (t>>7) + 2i.
  // B tile (16 x 64): n-fast -> nn = t&63, kk = (t>>6) + 4i; else kk = t&15, nn = (t>>4) + 16i.  The m / n offsets
  // do not depend on the K-slab: computed once.
  const bool a_kf = g.av.c_fast, b_nf = g.bv.c_fast;
  int64_t aoff[kLoadA], boff[kLoadB];
  uint32_t amask = 0, bmask = 0;
#pragma unroll
  for (int i = 0; i < kLoadA; ++i) {
    const int mm = a_kf ? (t >> 4) + 16 * i : (t & 127);
    const int m = m0 + mm;
    aoff[i] = m < g.M ? g.av.r.off(m) : 0;
    amask |= (m < g.M ? 1u : 0u) << i;
  }
#pragma unroll
  for (int i = 0; i < kLoadB; ++i) {
    const int nn = b_nf ? (t & 63) : (t >> 4) + 16 * i;
    const int n = n0 + nn;
    boff[i] = n < g.N ? g.bv.c.off(n) : 0;
    bmask |= (n < g.N ? 1u : 0u) << i;
  }
  double ra[kLoadA], rb[kLoadB];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < kLoadA; ++i) {
      const int k = k0 + (a_kf ? (t & 15) : (t >> 7) + 2 * i);
      const bool ok = ((amask >> i) & 1) && k < kend;
      ra[i] = ok ? g.a[aoff[i] + g.av.c.off(k)] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kLoadB; ++i) {
      const int k = k0 + (b_nf ? (t >> 6) + 4 * i : (t & 15));
      const bool ok = ((bmask >> i) & 1) && k < kend;
      rb[i] = ok ? g.b[boff[i] + g.bv.r.off(k)] : 0.0;
    }
  };

  f64x4 acc[4][2];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  if (kbeg < kend) fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += kGK) {
    __syncthreads();  // every wave is done reading the previous slab
#pragma unroll
    for (int i = 0; i < kLoadA; ++i) {
      const int mm = a_kf ? (t >> 4) + 16 * i : (t & 127), kk = a_kf ? (t & 15) : (t >> 7) + 2 * i;
      As[kk][mm] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < kLoadB; ++i) {
      const int nn = b_nf ? (t & 63) : (t >> 4) + 16 * i, kk = b_nf ? (t >> 6) + 4 * i : (t & 15);
      Bs[kk][nn] = rb[i];
    }
    __syncthreads();
    if (k0 + kGK < kend) fetch(k0 + kGK);  // in flight while the MFMAs below run
#pragma unroll
    for (int ks = 0; ks < kGK / 4; ++ks) {
      const int kr = ks * 4 + (lane >> 4);
      double fa[4], fb[2];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) fa[mi] = As[kr][wm + mi * 16 + (lane & 15)];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) fb[ni] = Bs[kr][wn + ni * 16 + (lane & 15)];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
  }

  double *part = g.part ? g.part + (int64_t)blockIdx.z * g.M * g.N : nullptr;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n0 + wn + ni * 16 + (lane & 15);
    if (n >= g.N) continue;
    const int64_t cn = part ? n : g.cv.c.off(n);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + (lane >> 4) + 4 * r;
        if (m >= g.M) continue;
        if (part) {
          part[(int64_t)m * g.N + cn] = acc[mi][ni][r];
        } else {
          double *p = g.c + g.cv.r.off(m) + cn;
          *p = g.beta ? *p + acc[mi][ni][r] : acc[mi][ni][r];
        }
      }
    }
  }
}

// Second pass of the split-K: C = beta*C + sum over slices, in slice order.
__global__ __launch_bounds__(256) void gemm_f64_reduce_kernel(const GemmArgs g, int slices) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)g.M * g.N) return;
  const int m = (int)(i / g.N), n = (int)(i - (int64_t)m * g.N);
  double s = 0.0;
  for (int z = 0; z < slices; ++z) s += g.part[(int64_t)z * g.M * g.N + i];
  double *p = g.c + g.cv.r.off(m) + g.cv.c.off(n);
  *p = g.beta ? *p + s : s;
}

// K per slice and number of slices.  split_k: 0 auto, 1 off, > 1 about that many slices (K rounded to kGK per slice).
// Auto: only when the output has too few tiles to fill the 256 CUs and K is long; about 1024 workgroups then.
void split_plan(int64_t M, int64_t N, int64_t K, int split_k, int64_t *k_slice, int64_t *slices) {
  int64_t want = split_k;
  if (split_k == 0) {
    const int64_t tiles = ceil_div(M, kGM) * ceil_div(N, kGN);
    want = (tiles >= 512 || K <= 1024) ? 1 : std::min(ceil_div(1024, tiles), ceil_div(K, 512));
  }
  want = std::max<int64_t>(1, std::min<int64_t>(want, 65535));
  int64_t ks = ceil_div(ceil_div(std::max<int64_t>(K, 1), want), kGK) * kGK;
  *k_slice = ks;
  *slices = ceil_div(std::max<int64_t>(K, 1), ks);
}

// View descriptor of the ABI: {row d0, d1, d2, s0, s1, s2, col d0, d1, d2, s0, s1, s2}; d0*d1*d2 = the extent
// (any sub-index sizes >= 1 for an empty extent).
int parse_view(const int64_t *v, int64_t rows, int64_t cols, View *out) {
  Axis *ax[2] = {&out->r, &out->c};
  const int64_t ext[2] = {rows, cols};
  for (int a = 0; a < 2; ++a) {
    const int64_t *d = v + 6 * a;
    if (d[0] < 1 || d[1] < 1 || d[2] < 1 || d[0] > INT32_MAX || d[1] > INT32_MAX || d[2] > INT32_MAX) return GFLA_ERR_BAD_SHAPE;
    if (ext[a] > 0 && d[0] * d[1] * d[2] != ext[a]) return GFLA_ERR_BAD_SHAPE;
    ax[a]->d1 = (uint32_t)d[1];
    ax[a]->d2 = (uint32_t)d[2];
    ax[a]->s0 = d[3];
    ax[a]->s1 = d[4];
    ax[a]->s2 = d[5];
  }
  auto inner = [](const int64_t *d) {  // |stride| of the fastest-varying sub-index that actually varies
    const int64_t s = d[2] > 1 ? d[5] : d[1] > 1 ? d[4] : d[3];
    return s < 0 ? -s : s;
  };
  out->c_fast = inner(v + 6) <= inner(v);
  return GFLA_OK;
}

}  // namespace
}  // namespace gfla

extern "C" {

int64_t gfla_gemm_f64_workspace_bytes(int64_t M, int64_t N, int64_t K, int split_k) {
  if (M < 0 || N < 0 || K < 0 || split_k < 0) return -1;
  int64_t ks, slices;
  gfla::split_plan(M, N, K, split_k, &ks, &slices);
  return slices > 1 ? slices * M * N * (int64_t)sizeof(double) : 0;
}

int gfla_gemm_f64(double *c, const int64_t *c_view, const double *a, const int64_t *a_view, const double *b,
                  const int64_t *b_view, int64_t M, int64_t N, int64_t K, int beta, int split_k, void *workspace,
                  gfla_stream_t stream) {
  using namespace gfla;
  if (!c || !c_view || !a || !a_view || !b || !b_view) return GFLA_ERR_NULL_POINTER;
  if (M < 0 || N < 0 || K < 0 || (beta != 0 && beta != 1) || split_k < 0) return GFLA_ERR_BAD_SHAPE;
  GemmArgs g{};
  if (int rc = parse_view(c_view, M, N, &g.cv)) return rc;
  if (int rc = parse_view(a_view, M, K, &g.av)) return rc;
  if (int rc = parse_view(b_view, K, N, &g.bv)) return rc;
  if (M > 0x7fffff00LL || N > 0x7fffff00LL || K > 0x7fffff00LL || ceil_div(M, kGM) > 65535) return GFLA_ERR_UNSUPPORTED;
  int64_t ks, slices;
  split_plan(M, N, K, split_k, &ks, &slices);
  if (slices > 1 && !workspace) return GFLA_ERR_NULL_POINTER;
  if (M == 0 || N == 0) return GFLA_OK;
  g.c = c;
  g.a = a;
  g.b = b;
  g.M = (int)M;
  g.N = (int)N;
  g.K = (int)K;
  g.beta = beta;
  g.k_slice = (int)ks;
  g.part = slices > 1 ? static_cast<double *>(workspace) : nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)ceil_div(N, kGN), (unsigned)ceil_div(M, kGM), (unsigned)slices);
  gemm_f64_kernel<<<grid, kGThreads, 0, st>>>(g);
  if (slices > 1) gemm_f64_reduce_kernel<<<(unsigned)ceil_div(M * N, 256), 256, 0, st>>>(g, (int)slices);
  const int rc = launch_status();
  if (rc == GFLA_OK) note_path(GFLA_PATH_GEMM_F64);
  return rc;
}

}  // extern "C"
