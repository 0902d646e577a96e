// The epilogue of a weight-gradient workgroup, dW = G^T dU G: the tail of fc_wino_wgrad_kernel and fc_wino16_wgrad_kernel,
// written once and #included into the body of each (fc_wino_wgrad.h says why it is text and not a function).
// C/D layout of the 16x16 MFMA: column (hidden channel) = lane & 15, row (input channel) = 4*(lane >> 4) + r: a lane holds
// ALL 36 points of its four (c, n) pairs, so it applies dW = G^T dU G itself and the split's partial leaves as k*k values
// per pair instead of 36 -- in the direct kernel's [split][tap][c][n] layout, which fc_wgrad_reduce sums straight into
// conv0.weight.grad (k = 3: a quarter of the partial traffic, k = 5: 70 %, and no separate transform pass; the transform
// is linear, so doing it per split changes rounding only).  It uses these names of the including kernel:
//   KS, acc, cpad, kq      kernel size, the 36 accumulators, padded input channels, lane >> 4
//   o                      the lane's column of the split's slab: row 4 * kq + r of tap (i, j) is o[((i KS + j) cpad + 4 kq + r) 128]
//   unscaled(v)            v times the inverse scales of the operands (two-term f16), or v itself -- no multiply at all
{
  // G (6 x k): G[a][i] = p_a^i / f_a for a < 5, G[5][k-1] = 1 (wn_g)
  constexpr float inv_f[5] = {1.f, -1.f / 3.f, 1.f / 3.f, 1.f / 15.f, -16.f / 15.f};
  constexpr float pt[5] = {0.f, 1.f, -1.f, 2.f, -0.5f};
  float G[6][KS];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    float pw = 1.f;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      G[a][i] = pw * inv_f[a];
      pw *= pt[a];
    }
  }
#pragma unroll
  for (int i = 0; i < KS; ++i) G[5][i] = i == KS - 1 ? 1.f : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float tmp[KS][6];
#pragma unroll
    for (int i = 0; i < KS; ++i)
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        float sum = 0.f;
#pragma unroll
        for (int a = 0; a < 6; ++a) sum += G[a][i] * acc[a * 6 + e][r];
        tmp[i][e] = sum;
      }
#pragma unroll
    for (int i = 0; i < KS; ++i)
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 6; ++e) sum += tmp[i][e] * G[e][j];
        o[((int64_t)(i * KS + j) * cpad + 4 * kq + r) * kFcHidden] = unscaled(sum);
      }
  }
}
