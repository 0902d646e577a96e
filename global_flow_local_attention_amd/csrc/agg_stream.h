// What agg_coef_kernel, agg_fwd_stream_kernel and agg_ga_stream_kernel (local_attn_aggregate.hip) share, each thing once:
// the interleaved-pair plane layout, the workgroup / lane decode, the double-buffered staging pipeline with its rules,
// the paired row reader, the per-axis tap arithmetic of pixels that are not a dense patch, and on the host side the launch
// geometry, the eligibility predicates and the chunk-size dispatch.
#pragma once
#include <algorithm>
#include <type_traits>

#include "gfla_common.h"

namespace gfla {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAggStreamWaves = 12;  // <= 12 waves per workgroup: the stream kernels hold ~170 VGPRs per lane
constexpr int kAggChunk = 4;  // channels whose accumulators one lane of agg_fwd_lds_kernel keeps in registers at a time
constexpr int kAggMaxChunk = 8;      // planes per chunk the stream kernels are instantiated for (2, 4, 6, 8)

// ---------------------------------------------------------------------------------------------- plane layout in LDS
// Rows in INTERLEAVED PAIRS,
//     word(y, x) = (y / 2) * pitch + (x / 2) * 4 + (y % 2) * 2 + (x % 2),     pitch = 32 (mod 64), >= 2 * Ws
// A word pair (even x) stays contiguous (one ds_read_b64), rows y and y+1 of a pair never share a bank (they occupy
// alternate 8-byte slots), and consecutive row pairs are 32 banks apart: a lane group whose addresses span <= 8 word
// pairs of <= 4 plane rows -- a 16 x 2 or 8 x 4 pixel tile with a coherent flow -- reads without bank conflicts (zero
// flow: 4 % conflict cycles; the bench's flow, which moves ~1 pixel per pixel, still loses 40 %, down from 60 % for
// row-major planes read by 64 pixels of one row).
__device__ __forceinline__ int agg_row_base(int yc, int pitch) { return (yc >> 1) * pitch + ((yc & 1) << 1); }  // word(yc, 0)
__device__ __forceinline__ int agg_col_word(int xc) { return ((xc >> 1) << 2) + (xc & 1); }                     // word(0, xc)
// first word of a row window that starts at the EVEN column xa (word pairs of a row sit 4 words apart)
__device__ __forceinline__ int agg_row_window(int yc, int xa, int pitch) { return agg_row_base(yc, pitch) + (xa << 1); }

// ------------------------------------------------------------------------------------- workgroup / lane decode, records
constexpr unsigned kAggNotDense = 0xffffffffu;  // packed word of a pixel whose taps are not a dense patch
constexpr unsigned kAggSkip = 0xfffffffeu;      // lane without a pixel (tile overhang)

template <int K>
constexpr int agg_coef_slots() { return (K + 1) * (K + 2); }
// floats per pixel in the table: the coefficients + the packed word, padded to whole 16-byte vectors -- a lane fetches
// its record with a few dwordx4 loads (the texture addresser spends ~16 cycles per wave load whatever its width: one
// dword load per coefficient was the bottleneck of the first version of this kernel)
constexpr int agg_record_floats(int k) { return ((k + 1) * (k + 2) + 1 + 3) & ~3; }

// wave <-> 64-pixel tile t of sample b, lane <-> pixel: the ONE mapping the coefficient writer and both stream kernels
// use (records land on the wrong pixels otherwise).  Stream kernels: workgroup <-> (sample, tile group tg = blockDim/64
// tiles, channel range sg = [c_begin, c_end)).
struct AggLane {
  int b, c_begin, c_end;  // sample; channel range of the workgroup (stream kernels)
  int t, lane, yf, xf, p;  // p = 0 for a lane without a pixel (loads through it stay in bounds)
  bool active;

  __device__ __forceinline__ void pixel(int tile, int tw_log2, int ntile, int H, int W) {
    t = tile;
    lane = threadIdx.x & 63;
    active = false;
    p = yf = xf = 0;
    if (t < ntile) {
      const int tw = 1 << tw_log2, th = 64 >> tw_log2, tiles_x = (W + tw - 1) >> tw_log2;
      const int ty = t / tiles_x, tx = t - ty * tiles_x;
      yf = ty * th + (lane >> tw_log2);
      xf = (tx << tw_log2) + (lane & (tw - 1));
      active = yf < H && xf < W;
      if (active) p = yf * W + xf;
    }
  }
  // stream kernels; false: a workgroup of the padding (the grid is rounded up to a multiple of kNumXCD).
  // Every XCD gets a contiguous run of the (sample, channel range, tile group) index space: the tile groups that stage
  // the same planes, and the channel ranges that read the same records, share one L2.
  __device__ __forceinline__ bool stream(int C, int CS, int nsuper, int tgroups, int total, int tw_log2, int ntile, int H,
                                         int W) {
    const int per_xcd = (total + kNumXCD - 1) / kNumXCD;
    int bid = (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD;
    if (bid >= total) return false;
    const int tg = bid % tgroups;
    bid /= tgroups;
    const int sg = bid % nsuper;
    b = bid / nsuper;
    c_begin = sg * CS;
    c_end = min(C, c_begin + CS);
    pixel(tg * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6), tw_log2, ntile, H, W);
    return true;
  }
  // the lane's record in the table, as f32x4 vectors laid out [sample][tile][vector][lane]: vector v is record<NR>()[v * 64]
  template <int NR, typename V>
  __device__ __forceinline__ V *record(V *table, int ntile) const {
    return table + ((int64_t)b * ntile + t) * (NR / 4) * 64 + lane;
  }
};

// -------------------------------------------------------------------------------------------------- staging pipeline
// A chunk of planes is moved in two halves so that the global loads of the NEXT chunk are in flight while the current
// one is being read: agg_chunk_load (global -> registers, word pairs) ... agg_chunk_store (registers -> LDS).
constexpr int kAggPre = 8;  // word pairs per thread and chunk (the launcher sizes the chunk accordingly)

template <typename T>
__device__ __forceinline__ void agg_chunk_load(const T *__restrict__ g, int n, f32x2 (&pre)[kAggPre]) {
#pragma unroll
  for (int j = 0; j < kAggPre; ++j) {
    // unconditional (index clamped): a load under `if (i < n)` turns into a branch + s_waitcnt per load
    const int i = min(j * (int)blockDim.x + (int)threadIdx.x, n - 1);
    if constexpr (sizeof(T) == 4) {
      pre[j] = reinterpret_cast<const f32x2 *>(g)[i];
    } else if constexpr (std::is_same<T, f16_t>::value) {
      const unsigned raw = reinterpret_cast<const unsigned *>(g)[i];  // two f16
      pre[j] = f32x2{Num<f16_t>::ld(reinterpret_cast<const f16_t *>(&raw)), Num<f16_t>::ld(reinterpret_cast<const f16_t *>(&raw) + 1)};
    } else {
      const unsigned raw = reinterpret_cast<const unsigned *>(g)[i];  // two bf16
      pre[j] = f32x2{__uint_as_float(raw << 16), __uint_as_float(raw & 0xffff0000u)};
    }
  }
}
// LDS word offsets of the thread's kAggPre word pairs inside a chunk buffer (the same for every chunk: computed once,
// two 16-bit offsets per register; the chunk buffer has < 2^16 words... in units of 2 words)
__device__ __forceinline__ void agg_chunk_offsets(int n_max, int per_plane, int wp, int pitch, int plane_sz,
                                                  unsigned (&off)[kAggPre / 2]) {
  const unsigned m_pl = 0xffffffffu / (unsigned)per_plane + 1u, m_wp = 0xffffffffu / (unsigned)wp + 1u;  // n * d < 2^32
#pragma unroll
  for (int j = 0; j < kAggPre; ++j) {
    const int i = min(j * (int)blockDim.x + (int)threadIdx.x, n_max - 1);
    const int c = (int)__umulhi((unsigned)i, m_pl);
    const int rem = i - c * per_plane;
    const int y = (int)__umulhi((unsigned)rem, m_wp);
    const int xp = rem - y * wp;
    const unsigned o = (unsigned)(c * plane_sz + agg_row_window(y, 2 * xp, pitch)) >> 1;  // even word -> /2
    if (j & 1) off[j >> 1] |= o << 16; else off[j >> 1] = o;
  }
}
__device__ __forceinline__ void agg_chunk_store(float *lds, int n, const f32x2 (&pre)[kAggPre],
                                                const unsigned (&off)[kAggPre / 2]) {
#pragma unroll
  for (int j = 0; j < kAggPre; ++j) {
    const int i = j * (int)blockDim.x + (int)threadIdx.x;
    const unsigned o = (j & 1) ? off[j >> 1] >> 16 : off[j >> 1] & 0xffffu;
    if (i < n) *reinterpret_cast<f32x2 *>(lds + 2 * o) = pre[j];
  }
}

// The channels [c_begin, c_end) of sample b stream through two LDS buffers in chunks of CH planes: prologue() stages the
// first chunk; per chunk, prefetch() puts the next chunk's loads in flight, the kernel reads planes(), commit() flips
// the buffers and stages the next chunk.
// The rules (each cost an exposed round trip per step when broken; found in the ISA of the first versions):
//   * the prefetch is UNCONDITIONAL -- the last chunk re-requests one word pair of its own first plane: with the loads
//     under a branch hipcc cannot count them, and every later wait for an older store becomes vmcnt(0), a wait for
//     these loads;
//   * the memory counter is in order: waiting for the YOUNGEST store waits for the prefetch as well.  So a kernel's
//     result stores go ONCE per chunk, behind commit()'s wait (which the staging needs anyway), never inside the
//     channel loop; they fly during the next chunk;
//   * commit() says vmcnt(0) unconditionally, and the rarely taken tap-by-tap branch, with loads of its own, says it on
//     its way out (agg_taps_done), so that nothing but those result stores is pending when the loop comes round;
//   * the barrier after commit() (the next chunk has landed, and nobody still reads the buffer the one after it will
//     overwrite) belongs to the kernel: it comes after the result stores.
// NO_STAGING: the forward kernel's timing ablation (GFLA_AGG_ABL bit 2; results are garbage).
template <typename T, bool NO_STAGING = false>
struct AggStage {
  float *lds;
  const T *s0;  // plane c_begin of the sample
  int CH, Hs, Ws, pitch, c_begin, c_end;
  int plane_sz, buf_sz, per_plane, cur;
  f32x2 pre[kAggPre];
  unsigned off[kAggPre / 2];

  __device__ __forceinline__ void prologue() {
    plane_sz = ((Hs + 1) >> 1) * pitch;
    buf_sz = CH * plane_sz + 4;  // + the word pair a window may read past the last row
    const int wp = Ws >> 1;      // word pairs per row (Ws is even)
    per_plane = Hs * wp;         // word pairs per plane
    cur = 0;
    agg_chunk_offsets(CH * per_plane, per_plane, wp, pitch, plane_sz, off);
    const int gc = min(CH, c_end - c_begin);
    agg_chunk_load<T>(s0, gc * per_plane, pre);
    const int nrow = CH * ((Hs + 1) >> 1);
    for (int u = 0; u < 2; ++u) {  // words no load ever writes must be finite: they meet weight 0 / are never selected
      float *bf = lds + u * buf_sz;
      if (pitch >= 2 * Ws + 4)
        for (int i = threadIdx.x; i < nrow * 4; i += blockDim.x) bf[(i >> 2) * pitch + 2 * Ws + (i & 3)] = 0.f;
      if (threadIdx.x < 4) bf[CH * plane_sz + threadIdx.x] = 0.f;
    }
    agg_chunk_store(lds, gc * per_plane, pre, off);
    __syncthreads();
  }
  // planes of the chunk after the one at cb (<= 0: none)
  __device__ __forceinline__ int next_planes(int cb) const { return min(CH, c_end - cb - CH); }
  __device__ __forceinline__ void prefetch(int cb, int gn) {
    if constexpr (!NO_STAGING)
      agg_chunk_load<T>(s0 + (int64_t)(gn > 0 ? cb + CH - c_begin : 0) * Hs * Ws, gn > 0 ? gn * per_plane : 1, pre);
  }
  __device__ __forceinline__ const float *planes() const { return lds + cur * buf_sz; }
  __device__ __forceinline__ void commit(int gn) {
    if constexpr (!NO_STAGING) {
      cur ^= 1;
      if (gn > 0) agg_chunk_store(lds + cur * buf_sz, gn * per_plane, pre, off);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
  }
};

// One row window of one plane: N ds_read_b64 from an even word.  The empty asm statements keep the reads apart: merged
// into ds_read2_b64 they would run at half the LDS rate (MI355X_MICROARCH.md, LDS table).
template <int N>
__device__ __forceinline__ void agg_load_row(const float *rp, f32x2 *v) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = *reinterpret_cast<const f32x2 *>(rp + 4 * i);
    asm volatile("" ::: "memory");
  }
}

// A pixel whose taps are not a dense patch (floor() of some tap landed one off: a flow within rounding of an integer;
// rare) is evaluated tap by tap, exactly as block_extractor does, in rolled loops (#pragma unroll 1) over the tap rows
// and columns so that the branch costs no registers.  One axis of tap t of K around pos + f0
// (block_extractor_kernel.cu:62-76): the clamped coordinates of its two neighbours and the weight of the upper one
// (the lower one's is 1 - w_hi).  The kernels spell the loads and the four-term sums out themselves: what hipcc
// contracts into FMAs, and in which operand order, changed when the sums sat in a callback of a shared walker.
struct AggTapAxis { int lo, hi; float w_hi; };
template <int K>
__device__ __forceinline__ AggTapAxis agg_tap_axis(float f0, int t, int pos, int n) {
  const float d = (f0 + (float)(t - K / 2)) + (float)pos;
  const float fd = floorf(d);
  return AggTapAxis{clampi((int)fd, 0, n - 1), clampi((int)(fd + 1), 0, n - 1), d - fd};
}
// On every path out of the tap-by-tap branch: its loads have all been consumed; saying so keeps them from turning
// the dense path's register reuse into waits for the prefetch.
__device__ __forceinline__ void agg_taps_done() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// ------------------------------------------------------------------------------------------------------- host side
// Launch geometry of the stream kernels.
struct AggStreamGeo {
  int CH, CS, nsuper, tgroups, threads, pitch, tw_log2, ntile;
  unsigned lds;
};
inline AggStreamGeo agg_stream_geometry(int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k) {
  AggStreamGeo g{0, 0, 1, 1, 0, 0, 4, 0, 0};
  // tile width: the one that wastes the fewest lanes on the overhang (16 on ties); tuning key 16 overrides
  int twl = 4;
  double best_eff = -1;
  for (int cand : {4, 3, 5}) {
    const int64_t tw = 1 << cand, th = 64 >> cand;
    const double eff = (double)(H * W) / (double)(ceil_div(W, tw) * tw * ceil_div(H, th) * th);
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      twl = cand;
    }
  }
  if (tuning(GFLA_TUNE_AGG_STREAM_TILE_W) == 8 || tuning(GFLA_TUNE_AGG_STREAM_TILE_W) == 16 ||
      tuning(GFLA_TUNE_AGG_STREAM_TILE_W) == 32)
    twl = tuning(GFLA_TUNE_AGG_STREAM_TILE_W) == 8 ? 3 : tuning(GFLA_TUNE_AGG_STREAM_TILE_W) == 16 ? 4 : 5;
  const int64_t ntile = ceil_div(W, 1 << twl) * ceil_div(H, 64 >> twl);
  // tiles (waves) per workgroup
  const int64_t tmax = tuning(GFLA_TUNE_AGG_STREAM_THREADS) >= 64 && tuning(GFLA_TUNE_AGG_STREAM_THREADS) <= kAggStreamWaves * 64
                           ? tuning(GFLA_TUNE_AGG_STREAM_THREADS) / 64 : kAggStreamWaves;
  const int64_t tgroups = ceil_div(ntile, tmax);
  const int64_t twg = ceil_div(ntile, tgroups);  // balanced
  const int64_t threads = twg * 64;
  int pitch = (int)(ceil_div(2 * Ws + 32, 64) * 64 - 32);  // smallest value >= 2 Ws that is 32 mod 64
  if (tuning(GFLA_TUNE_AGG_STREAM_PITCH) >= 2 * Ws && !(tuning(GFLA_TUNE_AGG_STREAM_PITCH) & 3))
    pitch = tuning(GFLA_TUNE_AGG_STREAM_PITCH);  // experiment: pair pitch in words
  const int64_t per_plane = ceil_div(Hs, 2) * pitch * 4;
  const int64_t budget = 160 * 1024 - 64;
  // chunk: as many planes as two buffers fit and kAggPre word pairs per thread cover
  int64_t CH = std::min<int64_t>((budget / 2 - 16) / per_plane, kAggPre * threads / (Hs * (Ws / 2)));
  if (CH > C) CH = C;
  if (CH > kAggMaxChunk) CH = kAggMaxChunk;   // the forward kernel keeps a chunk's results in registers
  if (tuning(GFLA_TUNE_G_CAP) > 0 && tuning(GFLA_TUNE_G_CAP) < CH) CH = tuning(GFLA_TUNE_G_CAP);
  if (CH >= 2) CH &= ~1LL;  // channel pairs
  if (CH < 1) return g;
  // channel ranges: more of them = more workgroups, fewer chunks each (the first chunk of a workgroup is not overlapped)
  int64_t best_ns = 1;
  double best_cost = -1;
  for (int64_t ns = 1; ns * CH <= C || ns == 1; ns *= 2) {
    const int64_t CS = ceil_div(ceil_div(C, ns), CH) * CH;
    const int64_t nsr = ceil_div(C, CS);
    const int64_t wgs = B * tgroups * nsr;
    const double rounds = (double)ceil_div(wgs, kNumCU);
    const double cost = rounds * (1.3 + (double)(CS / CH));
    if (best_cost < 0 || cost < best_cost - 1e-9) {
      best_cost = cost;
      best_ns = ns;
    }
  }
  if (tuning(GFLA_TUNE_SPLIT) > 0) best_ns = tuning(GFLA_TUNE_SPLIT);
  const int64_t CS = ceil_div(ceil_div(C, best_ns), CH) * CH;
  g = AggStreamGeo{(int)CH, (int)CS, (int)ceil_div(C, CS), (int)tgroups, (int)threads, pitch, twl, (int)ntile,
                   (unsigned)(2 * (CH * per_plane + 16))};
  return g;
}

// What makes the stream kernels CORRECT for source planes of Hs x Ws and kernel size k:
//   odd k                the paired reads are laid out for it (static_assert in the kernels)
//   Ws >= k + 1, even    the aligned row window [xa, xa + k + 2] lies inside the padded row; rows are staged in word pairs
//   Ws < 32768, Hs < 32000   window start and first row share one packed 32-bit word of the record (16 bits each, row + 16)
//   B C Hs Ws < 2^31     conservative (what spans the tensor is indexed in 64 bits); kept so that no call changes its path
// batch_in_grid_y: B <= 65535.  The coefficient pass puts the sample in blockIdx.y, so the forward and the geometry query,
// which describes the forward, need it; the stream kernels themselves decode the sample from blockIdx.x and do not.
inline bool agg_stream_shape_ok(int64_t B, int64_t C, int64_t Hs, int64_t Ws, int k, bool batch_in_grid_y) {
  return (k & 1) && Ws >= k + 1 && !(Ws & 1) && Ws < 32768 && Hs < 32000 && B * C * Hs * Ws < (1LL << 31) &&
         (!batch_in_grid_y || B <= 65535);
}
// (Policy -- whether the default dispatch wants them -- is gs_route.h: agg_stream_enabled / agg_stream_wanted.)

// Geometry + grid of a stream-kernel launch; false: no chunk fits LDS, or the padded grid overflows.
struct AggStreamPlan { AggStreamGeo pg; int64_t total, padded; };  // workgroups with work / launched (multiple of kNumXCD)
inline bool agg_stream_plan(int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k, AggStreamPlan &pl) {
  pl.pg = agg_stream_geometry(B, C, Hs, Ws, H, W, k);
  pl.total = B * pl.pg.nsuper * pl.pg.tgroups;
  pl.padded = ceil_div(pl.total, kNumXCD) * kNumXCD;
  return pl.pg.CH > 0 && pl.padded <= 0x7fffffffLL;
}

// CH (run time, 1..kAggMaxChunk) -> CHT, the compile-time planes per chunk of the instantiation that takes it
#define GFLA_AGG_CHT_SWITCH(CHV, ...)                                \
  if ((CHV) <= 2) { constexpr int CHT = 2; __VA_ARGS__; }            \
  else if ((CHV) <= 4) { constexpr int CHT = 4; __VA_ARGS__; }       \
  else if ((CHV) <= 6) { constexpr int CHT = 6; __VA_ARGS__; }       \
  else { constexpr int CHT = 8; __VA_ARGS__; }
// the odd kernel sizes the stream kernels are instantiated for (callers have checked agg_stream_shape_ok and k <= 5)
#define GFLA_AGG_ODD_K_SWITCH(KV, ...)                        \
  switch (KV) {                                               \
    case 1: { constexpr int K = 1; __VA_ARGS__; } break;      \
    case 3: { constexpr int K = 3; __VA_ARGS__; } break;      \
    default: { constexpr int K = 5; __VA_ARGS__; } break;     \
  }

}  // namespace gfla
