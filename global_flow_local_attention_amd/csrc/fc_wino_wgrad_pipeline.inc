// The unit / step pipeline of a weight-gradient workgroup: the loop of fc_wino_wgrad_kernel and fc_wino16_wgrad_kernel, written
// once and #included into the body of each (fc_wino_wgrad.h says why it is text and not a function).  Units [u0, u1) of the
// workgroup, 16 tiles per step.  The two halves of a step -- multiply this step's 16 tiles / transform the next 16 -- run in
// opposite order on the two waves of a SIMD; the next unit's raw rows are requested and written around the transform of the
// unit's first step.  It uses these names of the including kernel:
//   T, S               constexpr bool: with the transform / the staging (timing ablations run without; results are garbage)
//   xh, u0, u1         the wave's half (wave >> 2), the workgroup's units
//   walk, st           the WwWalk and the WwStage
//   first(un)          what the kernel requests before the first unit's raw rows are written
//   transform(half_tag, un, h, rbuf, vb)   raw buffer rbuf, step h of unit un -> V buffer vb
//   multiply(un, h, vb, un_next, h_next, any_next)   step h of un from V buffer vb; (un_next, h_next) is the step that
//                      follows, if any_next (the f16 kernel requests its dY there)
if (u0 < u1) {
    // prologue: raw of the first unit, V of its first step
    WwUnit cur = walk.unit_of(u0);
    st.prefetch(cur);
    first(cur);
    st.commit(cur, 0);
    __syncthreads();
    if (xh == 0) transform(Half0{}, cur, 0, 0, 0);
    else transform(Half1{}, cur, 0, 0, 0);
    __syncthreads();
    int vb = 0, rbuf = 0;
    for (int64_t u = u0; u < u1; ++u) {
      const int nh = (cur.nt + 15) >> 4;
      const bool has_next = u + 1 < u1;
      const WwUnit nxt = has_next ? walk.unit_of(u + 1) : cur;
      for (int h = 0; h < nh; ++h) {
        const bool last_h = h + 1 == nh;
        // the transform half of this step prepares the unit's next 16 tiles, or (last step of a two-step unit) the next
        // unit's first 16 -- whose raw rows were written during the unit's first step
        const bool t_same = T && !last_h, t_next = T && last_h && has_next && nh > 1;
        const bool stage = S && h == 0 && has_next;   // the next unit's raw rows: requested / written around the transform
        // the step that follows this one
        const bool any_next = !last_h || has_next;
        const WwUnit &dn = last_h ? nxt : cur;
        const int hn = last_h ? 0 : h + 1;
        if (xh == 0) {
          multiply(cur, h, vb, dn, hn, any_next);
          __builtin_amdgcn_sched_barrier(0);
          if (stage) st.prefetch(nxt);
          if (t_same) transform(Half0{}, cur, h + 1, rbuf, vb ^ 1);
          else if (t_next) transform(Half0{}, nxt, 0, rbuf ^ 1, vb ^ 1);
          if (stage) st.commit(nxt, rbuf ^ 1);
        } else {
          if (stage) st.prefetch(nxt);
          if (t_same) transform(Half1{}, cur, h + 1, rbuf, vb ^ 1);
          else if (t_next) transform(Half1{}, nxt, 0, rbuf ^ 1, vb ^ 1);
          if (stage) st.commit(nxt, rbuf ^ 1);
          __builtin_amdgcn_sched_barrier(0);
          multiply(cur, h, vb, dn, hn, any_next);
        }
        __syncthreads();
        if (last_h && has_next && nh == 1) {
          // a unit of ONE step: the next unit's raw rows were written during this very step, so its first transform runs
          // here, between two barriers (k = 3 layers and narrow maps: one exposed transform per unit)
          if constexpr (T) {
            if (xh == 0) transform(Half0{}, nxt, 0, rbuf ^ 1, vb ^ 1);
            else transform(Half1{}, nxt, 0, rbuf ^ 1, vb ^ 1);
          }
          __syncthreads();
        }
        vb ^= 1;
      }
      cur = nxt;
      rbuf ^= 1;
    }
}
