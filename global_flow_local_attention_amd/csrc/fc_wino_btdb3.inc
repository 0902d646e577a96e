// Rows 3*HALF .. 3*HALF + 2 of B^T d B for one transform item: the column and row passes of the four Winograd-domain kernels,
// written once and #included into each kernel's transform (fc_wino_shared.h says why it is text and not a function).  Only the
// three rows the wave group owns: 18 live values, half the column-pass arithmetic.  It uses these names of the including code:
//   HALF, PITCH        constexpr: the wave group's half of the point rows; LDS bytes per raw pixel
//   src, row_pitch     pixel (i, j) of the item's 6 x 6 window is the float at src + (i * row_pitch + j) * PITCH bytes (row_pitch:
//                      the map's Wp in the convolution kernels, the pitch of a unit's raw rows in the weight-gradient kernels)
//   store_row(r, o)    gets the six values of row r: the kernel's V layout, and the split into f16 terms where it has one
{
  __builtin_amdgcn_s_setprio(3);  // the short phase goes first whenever both waves of the SIMD can issue
  // column pass on PAIRS of columns: the same fma chain for columns j, j + 1 is one v_pk_fma_f32 / v_pk_add_f32 each
  // (vector instructions add to the MFMA time of the float32 kernels, so half as many of them is worth having)
  float tm[3][6];
#pragma unroll
  for (int jp = 0; jp < 3; ++jp) {
    f32x2v d[6], o[3];
#pragma unroll
    for (int i = 0; i < 6; ++i)
      d[i] = f32x2v{*reinterpret_cast<const float *>(src + (i * row_pitch + 2 * jp) * PITCH),
                    *reinterpret_cast<const float *>(src + (i * row_pitch + 2 * jp + 1) * PITCH)};
    wn_bt3<HALF, f32x2v>(d, o);
#pragma unroll
    for (int r = 0; r < 3; ++r) tm[r][2 * jp] = o[r][0], tm[r][2 * jp + 1] = o[r][1];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float o[6];
    wn_bt_pk(tm[r], o);
    store_row(r, o);
  }
  __builtin_amdgcn_s_setprio(0);
}
