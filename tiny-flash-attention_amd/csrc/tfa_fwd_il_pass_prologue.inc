// tfa_fwd_il_pass_prologue.inc — per-pass prologue of the issue-interleaved forward kernel: K(0), V(0), K(1) by LDS-DMA, Q fragments, S(0) and its row max
// A TEXTUAL piece of fwd_kernel_il (tfa_fwd_kernel_il.h includes it inside the kernel body, inside the pass loop): it is not a
// translation unit of its own and uses the kernel's locals.  Split out in round 3 without touching a token of the code — any edit
// here moves hipcc's schedule of the tile loop, so changes are judged by a same-process A/B (tools/ab_multi.py), never by eye.
    // ---- prologue: K(0), V(0), K(1) by DMA, Q fragments, S(0) and its row max -------------------------
    if (SEAM && seam_in) { /* the previous pass streamed K(0), K(1), V(0) and asked for Q */ }
    else if (PREF2) { /* requested and waited for in front of the pass loop (first pass) / at the end of the previous epilogue */ }
    else if (QLDS && pass == 0) { issue_first(mb); asm volatile("s_setprio 0" ::: "memory"); }
    else if (!PREF || pass == 0) { issue_prologue(mb, true); asm volatile("s_setprio 0" ::: "memory"); }      // (with PREF the previous pass already asked for this block)
    // this pass continues its tile stream into the next one when there is one and the buffer parities line up (nt even)
    const bool seam = SEAM && (pass + 1 < npass) && ((nt & 1) == 0) && nt >= 2;
    if (!PREF2) o_zero<DT>();                          // (PREF2: in front of the waits — before the pass loop / at the end of the previous epilogue)

    if (PREF2) {
      // K(0), V(0), K(1) and Q were requested and waited for before this point on EVERY path into the pass — in front of the pass loop,
      // or before the previous pass's O stores with a counted vmcnt behind them (end of that epilogue) — so that hipcc's own
      // wait-count model sees the Q registers complete at the loop header and adds no wait (which would be a wait for the stores)
    } else {
#if defined(TFA_IL_TRACEPRO)
      if (P_TRACE && pass == 0) {
        tp_issue = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DS) : "memory");
        tp_kv = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tp_q = __builtin_amdgcn_s_memtime();
      }
#endif
      if (QLDS && pass == 0) { wait_first(); read_q_lds(); }
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int s = 0; s < DS; ++s) asm volatile("" : "+v"(qf[s]));
    }
#if defined(TFA_IL_TRACEPRO)
    if (P_TRACE && pass == 0) tp_bar = __builtin_amdgcn_s_memtime();
#endif
    asm volatile("s_barrier" ::: "memory");
    if (P_TRACE && pass == tr_pass) t_pro = __builtin_amdgcn_s_memtime();

    // tiles this wave computes: 0 .. nact-1 (causal: the waves of a block stop at different tiles)
    const int nact = (wave_last_tile + 1 < nt_own) ? (wave_last_tile + 1) : nt_own;
    // A wave whose 32 rows all lie behind the last query row computes nothing: decode-like problems have one valid wave per
    // block, and the tile rate — hence the K/V streaming rate — is then that one wave's.  (A separate flag, not a smaller
    // nact: non-causal kernels keep nact == nt as a compile-time fact and lose 2 % without it.)
    const bool idle_wave = (VF & VF_IL_IDLE) != 0 && wave_row0 >= p.Nq;
    // first tile of this wave that needs masking (causal diagonal or ragged tail); nact if none
    int fm = nact;
    {
      int first_g = 0x3fffffff;                            // first tile OF THE HEAD that needs a mask for this wave
      if (IL_NK % BN) first_g = IL_NK / BN;
      if (CAUSAL) {
        const int c = pos_lo + shift + 1;                  // keys 0..c-1 are visible to every row of the wave
        const int full = c > 0 ? c / BN : 0;               // tiles 0..full-1 need no mask
        first_g = full < first_g ? full : first_g;
      }
      const int first = KSPLIT ? (first_g <= grp ? 0 : (first_g - grp + 1) >> 1) : first_g;   // ... in the wave's own tile numbering
      fm = first < fm ? first : fm;
    }

    f32x16 sA[2], sB[2];
    // (defined by an empty asm: hipcc otherwise gives the not-yet-written accumulators a value — 64 v_mov of zeros per workgroup, behind the wait)
    asm volatile("" : "=v"(sA[0]), "=v"(sA[1]), "=v"(sB[0]), "=v"(sB[1]));
    float mA = -INFINITY, mB = -INFINITY;
    auto qk_burst = [&](int kbuf, int t, f32x16 (&s)[2], float& mout) {   // S(t) = K(t) Q^T from K buffer kbuf, masked, row max
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[tt][r] = 0.f;
      const unsigned kb = kbuf * TILE_BYTES;
      u32x4 bq[4];                                       // BIAS: the tile's bias, requested ahead of the MFMAs
      if constexpr (BIAS) bias_issue(t, bq);
#pragma unroll
      for (int i = 0; i < N1; ++i) s[KT(i)] = E::mfma(k_frag_rt(kb, i), qf[KS(i)], s[KT(i)]);
      if constexpr (BIAS) bias_add(t, s, bq);
      else if constexpr (SMOD) apply_bias(t, s);
      if (needs_mask(t)) apply_mask(t, s);
      float mx = s[0][0];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[tt][r]);
      mout = pair_max(mx);
    };
    if (nact > 0 && !idle_wave) {
      qk_burst(0, 0, sA, mA);
      mref = fmaxf(mref, mA * sc);                       // first re-base for free: O = 0 and l = 0 so far
    }
    if constexpr (MAXFREE) {                             // a redone pass: the rows' true maxima, left in LDS by the redo's pre-pass (tfa_fwd_kernel_il.h)
      if (seeded) {
        const int l_ = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        mref = fmaxf(mref, reinterpret_cast<volatile float*>(smem + SEED_OFF)[wave_id * 32 + (l_ & 31)]);
      }
    }
    // K buffer 0 is refilled with K(2) at the top of iteration 0: every wave must be done with K(0)
    // (QLDS, first pass: V(0) and K(1) were left in flight behind S(0) — every wave's pieces must have landed before iteration 0 reads them.
    //  Not on a later pass: vmcnt(0) there would wait for the previous epilogue's O stores)
    if (QLDS && pass == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

#if defined(TFA_IL_TRACEWAIT)
    // debug build: split the end of an iteration into (memory wait) and (barrier) and sum the cycles of each
    auto iter_end = [&]() {
      const unsigned long long a0 = __builtin_amdgcn_s_memtime();
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const unsigned long long a1 = __builtin_amdgcn_s_memtime();
      asm volatile("s_barrier" ::: "memory");
      const unsigned long long a2 = __builtin_amdgcn_s_memtime();
      tw_wait += a1 - a0;
      tw_bar += a2 - a1;
    };
#elif defined(TFA_IL_TRACEITER)
    // debug build (tools/trace_diag.py): every wave stamps the end of each iteration that runs OUTSIDE the hand-scheduled loop — the loop's exit, the
    // compiler-scheduled bodies behind it (the diagonal), the idle iterations — into its slice of the idle epilogue region; dumped behind the tile loop
    int it_n = 0;
    auto it_stamp = [&](int tag) {
      if (P_TRACE && pass == tr_pass && it_n < 16) {
        typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
        const u32x2 rec = {(unsigned)__builtin_amdgcn_s_memtime(), (unsigned)tag};
        *reinterpret_cast<lds_u32x2*>(q_slice + it_n * 8) = rec;
        ++it_n;
      }
    };
    it_stamp(0);
    auto iter_end = [&]() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); it_stamp(2); };
#else
    auto iter_end = [&]() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
#endif

