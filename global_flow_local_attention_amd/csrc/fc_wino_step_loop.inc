// The steps of a convolution workgroup, two per 16-channel chunk: the loop of fc_wino_conv_kernel and fc_wino16_conv_kernel,
// written once and #included into the body of each (fc_wino_shared.h says why it is text and not a function).  It uses these
// names of the including kernel:
//   DB, DBG            template parameters: two raw buffers; timing ablations (1 no transform, 2 no multiply, 8 no raw staging)
//   xh, nch            the wave's half (wave >> 2), the input chunks
//   st                 the WnStage: chunk 0 is staged (prefetch(0), commit(0)), the first B fragments are requested
//   multiply(s, sn)    step s on the matrix cores, B fragments of step sn requested
//   transform(half_tag, step)   raw -> V[step & 1], the point rows of the wave's half
//   stamp(slot)        called behind the prologue (0), each half (1, 2) and the barrier (3): the float32 kernel's phase timing
// Waves w and w + 4 sit on the same SIMD and run the two halves of a step in OPPOSITE order -- one multiplies while the other
// transforms the next step's input (vector ALUs, LDS), so that the LDS / global latencies of one sit under the arithmetic of
// the other.
{
  constexpr bool kT = !(DBG & 1), kM = !(DBG & 2), kS = !(DBG & 8);
  const int nsteps = 2 * nch;
  __syncthreads();
  if (xh == 0) transform(Half0{}, 0);
  else transform(Half1{}, 0);
  __syncthreads();
  stamp(0);
  for (int s = 0; s < nsteps; ++s) {
    const int cc = s >> 1;
    const int sn = min(s + 1, nsteps - 1);
    // raw staging: the next chunk is requested and written inside the even step, around the transform (its registers are
    // live across the transform only; the loads have its duration to land).  Two raw buffers: no extra barrier.
    const bool stage_next = !(s & 1) && cc + 1 < nch;
    // (the transform of the step after the last one reads a stale raw buffer into the unused V buffer: harmless)
    // request, transform and write of the next chunk's pixels in ONE branch: as two separate `if (stage_next)` around a shared
    // transform hipcc cannot see that the write always follows the request, keeps the staging registers "pending" at the loop
    // header and opens the next request with s_waitcnt vmcnt(4) .. vmcnt(0) -- a wait for the B fragments the multiply half
    // requested a moment earlier (seen in the ISA in round 6; the float32 kernel had carried it since round 3)
    if (xh == 0) {
      if constexpr (kM) multiply(s, sn);
      __builtin_amdgcn_sched_barrier(0);
      stamp(1);
      if (kS && stage_next) {
        st.prefetch(cc + 1);
        if constexpr (kT) transform(Half0{}, s + 1);
        if constexpr (DB) st.commit(cc + 1);
      } else {
        if constexpr (kT) transform(Half0{}, s + 1);
      }
      stamp(2);
    } else {
      if (kS && stage_next) {
        st.prefetch(cc + 1);
        if constexpr (kT) transform(Half1{}, s + 1);
        if constexpr (DB) st.commit(cc + 1);
      } else {
        if constexpr (kT) transform(Half1{}, s + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      stamp(1);
      if constexpr (kM) multiply(s, sn);
      stamp(2);
    }
    __syncthreads();
    if constexpr (kS && !DB) {
      if (stage_next) {  // single raw buffer: written between two barriers (large maps only)
        st.commit(cc + 1);
        __syncthreads();
      }
    }
    stamp(3);
  }
}
