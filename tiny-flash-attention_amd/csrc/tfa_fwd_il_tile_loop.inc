// tfa_fwd_il_tile_loop.inc — the tile loop of the issue-interleaved forward kernel: the pinned fast path (fused), the burst-structured slow path, the loop over a wave's tiles
// A TEXTUAL piece of fwd_kernel_il (tfa_fwd_kernel_il.h includes it inside the kernel body, inside the pass loop): it is not a
// translation unit of its own and uses the kernel's locals.  Split out in round 3 without touching a token of the code — any edit
// here moves hipcc's schedule of the tile loop, so changes are judged by a same-process A/B (tools/ab_multi.py), never by eye.
    // ---- fast path: tile j (S in scur) -> O; S(j+1) and its row max -> snext, mnext.  One basic block. ---------
    // PAR = j & 1: K(j+1) is in K buffer PAR^1, V(j) in V buffer PAR; K(j+2) -> K buffer PAR, V(j+1) -> V buffer PAR^1.
    // RESC (EXACT only): some row's running maximum moved with tile j — O *= alpha rides behind the QK^T MFMAs, four registers per MFMA (N1 * 4 = 16 * DT)
    auto fused = [&](auto par_c, auto mask_c, auto resc_c, float alpha, int j, f32x16 (&scur)[2], f32x16 (&snext)[2], float& mnext) {
      constexpr int PAR = decltype(par_c)::value;
      constexpr bool MASK = decltype(mask_c)::value;   // tile j+1 is the wave's masked (diagonal / ragged) tile
      constexpr bool RESC = decltype(resc_c)::value;
      static_assert(!RESC || N1 * 4 == 16 * DT, "one O register quad per QK^T MFMA");
      constexpr bool SPREAD = (VF & VF_IL_DMASPREAD) != 0;
      constexpr bool STAGGER = SPREAD && (VF & VF_IL_DMASTAGGER) != 0;
      const bool late = STAGGER && wave >= NW / 2;
      const bool issue_k = (j + 2 < nt) || seam;         // beyond the last tile: the next pass's K(0) / K(1)
      const int tk = (j + 2 < nt) ? j + 2 : j + 2 - nt;
      if (!SPREAD && !(AB & ILAB_NODMA)) {
        if (issue_k) dma_k(tk, PAR);
        dma_v(j + 1, PAR ^ 1);
      }
      u32x4 bq[4];                                    // BIAS: tile j+1's bias, requested ahead of the QK^T MFMAs
      if constexpr (BIAS) bias_issue(j + 1, bq);
      const float msc = mref;
      constexpr int KB = PAR ^ 1;
      const char* vbp = vl + PAR * TILE_BYTES;
      unsigned pw[16];
      float xs[32];
      X8 kf[N1], vf[N2];
#pragma unroll
      for (int i = 0; i < PFK; ++i) kf[i] = k_frag(KB, i);
      // global MFMA slot g = 0..N1+N2-1; element e is summed/packed in slot SC(e), exponentiated in SC(e)-1, scaled in SC(e)-2
      auto soft_slot = [&](int g) {
#pragma unroll
        for (int e = 0; e < 32; ++e) {
          const int sc_e = slot_of_elem(e);
          const int sb_e = sc_e - 1, sa_e = sc_e >= 2 ? sc_e - 2 : 0;
          if (AB & ILAB_NOEXP) {
            if (sc_e == g && (e & 1)) pw[e >> 1] = __builtin_bit_cast(unsigned, scur[e >> 4][e & 15]);
          } else {
            if (sa_e == g) st_fma(e, scur, msc, xs);
            if (sb_e == g) st_exp(e, xs);
            if (sc_e == g) st_sum(e, xs, l4, pw);
          }
        }
      };
      __builtin_amdgcn_sched_barrier(0);
      // part 1
#pragma unroll
      for (int i = 0; i < N1; ++i) {
        if (i + PFK < N1) kf[i + PFK] = ((AB & ILAB_NOKREAD) && i + PFK >= PFK) ? kf[(i + PFK) % PFK] : k_frag(KB, i + PFK);
        else vf[i + PFK - N1] = v_frag(vbp, i + PFK - N1);
        if (AB & ILAB_NOQK) {
          if (i < 2) asm volatile("" : "+v"(snext[i]));
        } else if (KS(i) == 0) {                           // first k-slot of a key block: C = 0 (inline constant)
          f32x16 z;
#pragma unroll
          for (int r = 0; r < 16; ++r) z[r] = 0.f;
          snext[KT(i)] = E::mfma(kf[i], qf[KS(i)], z);
        } else {
          snext[KT(i)] = E::mfma(kf[i], qf[KS(i)], snext[KT(i)]);
        }
        if (SPREAD && !(AB & ILAB_NODMA) && !(STAGGER && late)) {   // 2*PPW DMA pieces spread over the first MFMAs, one per MFMA
          if (i < PPW) dma_v1(j + 1, PAR ^ 1, i);
          else if (i < 2 * PPW) { if (issue_k) dma_k1(tk, PAR, i - PPW); }
        }
        soft_slot(i);
        if constexpr (RESC) o_scale4_d(i, alpha);
        TFA_IL_PAD_HERE
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (SMOD) {                           // the cap and / or the bias in front of the mask and of the row maximum, on every tile
        if constexpr (BIAS) bias_add(j + 1, snext, bq);
        else apply_bias(j + 1, snext);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (MASK) {                                     // S(j+1) is complete (MFMA results: the s_nop covers the read distance)
        apply_mask(j + 1, snext);
        __builtin_amdgcn_sched_barrier(0);
      }
      // part 2
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < N2; ++i) {
        if (i + PFV < N2) vf[i + PFV] = (AB & ILAB_NOVREAD) ? vf[(i + PFV) % PFV] : v_frag(vbp, i + PFV);
        if (!(AB & ILAB_NOPV)) o_mfma_d<T>(i % DT, vf[i], p_frag(pw, i / DT));
        else asm volatile("" ::"v"(vf[i]), "v"(pw[(i / DT) * 4]), "v"(pw[(i / DT) * 4 + 1]), "v"(pw[(i / DT) * 4 + 2]), "v"(pw[(i / DT) * 4 + 3]));
        if (STAGGER && late && !(AB & ILAB_NODMA)) {
          if (i < PPW) dma_v1(j + 1, PAR ^ 1, i);
          else if (i < 2 * PPW) { if (issue_k) dma_k1(tk, PAR, i - PPW); }
        }
        soft_slot(N1 + i);
#pragma unroll
        for (int q = 0; q < 16; ++q)               // 16 pairs of S(j+1) values -> one v_max3 each
          if (q * N2 / 16 == i && !(AB & ILAB_NOMAX)) {
            mx = fmaxf(fmaxf(mx, snext[q >> 3][2 * (q & 7)]), snext[q >> 3][2 * (q & 7) + 1]);
            asm volatile("" : "+v"(mx));
          }
        TFA_IL_PAD_HERE
        __builtin_amdgcn_sched_barrier(0);
      }
      mnext = (AB & ILAB_NOMAX) ? snext[0][0] * 1e-30f : mx;   // this half-wave's 32 keys only (see rescale_if_needed)
      if (AB & ILAB_NOBARRIER) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else iter_end();
    };
    // ---- slow path: any tile (masked, last, re-base needed).  S(j) is in scur, S(j+1) goes to snext ------------------
    auto slow = [&](int j, f32x16 (&scur)[2], float mcur, f32x16 (&snext)[2], float& mnext) {
      const int par = j & 1;
      ++n_slow;
      if (j + 2 < nt) dma_k(j + 2, par);
      else if (seam) dma_k(j + 2 - nt, par);
      if (j + 1 < nt) dma_v(j + 1, par ^ 1);
      else if (seam) dma_v(0, par ^ 1);
      rescale_if_needed(mcur);
      const float msc = mref;
      const char* vbp = vl + par * TILE_BYTES;
      unsigned pw[16];
      float ev_hold = 0.f;
#pragma unroll
      for (int e = 0; e < 32; ++e) soft_elem(e, scur, msc, l4, pw, ev_hold);
#pragma unroll
      for (int i = 0; i < N2; ++i) o_mfma_d<T>(i % DT, v_frag(vbp, i), p_frag(pw, i / DT));
      if (j + 1 < nact) qk_burst(par ^ 1, j + 1, snext, mnext);
      iter_end();
    };

    // S(j) lives in sA for even j and in sB for odd j, on both paths, so the paths alternate freely without copies.
    // Tile j takes the fast path when tile j+1 exists and no row max of tile j has outgrown mref; if tile j+1 needs
    // masking (at most the wave's last one or two tiles) the body with the mask between its two parts runs.
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using MN = std::integral_constant<bool, false>;
    using MY = std::integral_constant<bool, true>;
    // ---- the hand-scheduled steady state (tfa_fwd_il_asm_loop.inc, generated by tools/gen_il_asm_loop.py): every instantiation with one descriptor per
    // slice and no idle-wave handling: 128 and 64 wide, 8-wave, 4-wave and key-split (the headline; its exact-running-max form at 128 wide x 8 waves).  From an EVEN tile j it runs tiles j, j+1, .. while the tile behind the current one
    // exists, needs no mask, has a whole K tile two ahead to request (j + 2 < nt_full) and no row has outgrown its reference; it returns the first tile it did not
    // process (either parity), S of that tile in sA / sB by parity, its half-wave row maximum in mx.  Everything else — masked and last tiles, re-bases,
    // odd entries — stays with the compiler-scheduled bodies below.
    constexpr bool ASMBASE = (D == 128 || D == 64) && DVB == D / 32 && (AB & ~ILAB_TRACE) == 0 && !WIN && !PAGED && !(VF & VF_IL_IDLE) && !(VF & (VF_IL_DMASTAGGER | VF_IL_SEAM)) &&
                             (PPW == 1 || PPW == 2 || PPW == 4) && (!EXACT || (D == 128 && PPW == 2)) && TFA_IL_USE_ASMLOOP && !SMOD;   // (the statement carries no bias and no cap)
    constexpr bool ASMLOOP = ASMBASE && !EXACT;        // the lazy-reference loop
    constexpr bool ASMLOOPX = ASMBASE && EXACT;        // the exact-running-max loop (variant 38): four bodies — parity x {plain, also re-basing O}
    // (the loop's LDS-DMA requests carry the tile's byte offset as their SCALAR offset, which the descriptor's bounds check does not see: it only asks for
    //  tiles that lie wholly inside the key sequence — K(j+2) with j + 2 < nt_full; a ragged last tile is requested by the compiler-scheduled bodies)
    const int nt_full = own_tiles(IL_NK / BN) < nt ? own_tiles(IL_NK / BN) : nt;     // (key-split kernels: in the wave group's own tile numbering)
    // ---- the bodies BEHIND the loop by hand as well (round 6): per wave and pass hipcc still scheduled the tile in front of the masked one, the masked tile and the
    // last one — on the causal diagonal, where half of the block's waves have already stopped, those iterations ran SLOWER than a steady-state one
    // (3000-3160 cycles against 2600, profiles/r06_trace_diag.txt).  The lazy-reference statement now carries them (dispatch + pinned / masked / last-tile body
    // per parity) and runs from any even tile without a pending re-base to the wave's last tile, leaving only for a re-base.  Their LDS-DMA requests carry the
    // tile offset as the SCALAR offset like the loop's, so the tails are on only while every tile of the block lies wholly inside the keys (nt_full == nt)
    // (key-split kernels too: a wave group has at most ONE masked tile in its own numbering — a 32-row wave straddles at most two tiles of the head, one per
    //  group — so the masked body's limit never advances there; a group whose last own tile does not exist fails nt_full == nt and keeps the tails off)
    constexpr bool ASMTAIL = (ASMLOOP || ASMLOOPX) && TFA_IL_USE_ASMTAIL;
    const bool tail_on = ASMTAIL && !seam && nt_full == nt;
    auto loop_ok = [&](int j) -> bool { return j + 1 < nact && j + 1 < fm && j + 2 < nt_full; };   // the loop proper takes tile j
    // LOCAL: the statement masks only the right edge — it is entered at tile j only when S(j+1) on needs no left mask (tiles 0 .. nlm-1 hold keys left of
    // the window of the wave's last row: the compiler-scheduled path computes their S through qk_burst's full mask)
    int nlm = 0;
    if (LOCAL) { const int e = pos_hi + shift - wlen; nlm = e > 0 ? (e + BN - 1) / BN : 0; }
    // EXACT: every tile with a successor takes the pinned body; the running maximum is advanced in front of it (exact_step) and the body that
    // also re-bases O runs when some row of the wave moved
    auto fast_exact = [&](auto par_c, bool masked, int j, f32x16 (&scur)[2], float mcur, f32x16 (&snext)[2], float& mnext) {
      float alpha;
      // (with the hand-scheduled loop in the kernel — ASMLOOPX — the unmasked pinned bodies would only serve the odd tile or two per pass the loop
      //  leaves behind: those go to the burst-structured path instead, four instantiations of the body and their registers less)
      if constexpr (ASMLOOPX) {
        if (!masked) { slow(j, scur, mcur, snext, mnext); return; }
        rescale_if_needed(mcur);                       // (the wave's one masked tile per pass: O re-based in a burst in front of the plain masked body)
        fused(par_c, MY{}, MN{}, 1.f, j, scur, snext, mnext);
        return;
      }
      if (exact_step(mcur, alpha)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) l4[i] *= alpha;
        if (!masked) fused(par_c, MN{}, MY{}, alpha, j, scur, snext, mnext);
        else fused(par_c, MY{}, MY{}, alpha, j, scur, snext, mnext);
      } else {
        if (!masked) fused(par_c, MN{}, MN{}, 1.f, j, scur, snext, mnext);
        else fused(par_c, MY{}, MN{}, 1.f, j, scur, snext, mnext);
      }
    };
    // the early requests for a pair's second pass (tfa_fwd_kernel_il.h: issue_early): in this pass's last iteration, by every wave — inside the idle loop below, or,
    // for a wave whose last tile IS the block's last, between two entries of the statement (xl = 1: it leaves in front of that tile; xl = 2: that tile, no vmcnt wait)
    const bool early_ok = PREF2 && ASMLOOP && TFA_IL_USE_EARLY && tail_on && pass + 1 < npass && (nt & 1) == 0 && nt >= 2;
    bool early_done = false, last_pending = false;
    auto asm_loop = [&](int& j, int xl_in) {
      if constexpr (ASMLOOP) {
        const int xl = __builtin_amdgcn_readfirstlane(xl_in);
        const int lim_t = fm < nact ? fm : nact;
        const int jend = (lim_t - 1 < nt_full - 2) ? lim_t - 1 : nt_full - 2;   // tiles j < jend take the loop
        int koff = (j + 2) * k_tile_stride, voff = (j + 1) * v_tile_stride;   // byte offset of the tile the next K / V request asks for
        const unsigned vaddr = lds_base + (unsigned)v_rd_base;
        const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds_base + wave * (PPW * 1024));
        float thr;
        u32x4 f0, f1, f2, f3, ka;
        unsigned ka5, ka6, ka7;
        // the tails' operands: the wave's and the block's tile counts, the first masked tile (-1: tails off) and the scalar part of the lanes' mask limit for it
        const int nact_s = __builtin_amdgcn_readfirstlane(nact), nt_s = __builtin_amdgcn_readfirstlane(nt);
        const int fmx = __builtin_amdgcn_readfirstlane(tail_on ? fm : -1);
        int ts;
        const int slim = __builtin_amdgcn_readfirstlane(wave_row0 + shift - key0_of(fm));   // (the lane adds its row inside the wave - 4 * its half-wave index)
        constexpr bool BF = std::is_same<T, __bf16>::value;      // one text per (kernel width, DMA pieces per wave, dtype)
        if constexpr (MAXFREE) {                             // (bf16 by definition: the texts without the row maximum)
          if constexpr (D == 128 && PPW == 2) { TFA_IL_ASM_LAZY_STMT(TFA_IL_ASM_LOOP_MF); }
          else if constexpr (D == 128) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D128_P4_MF, TFA_IL_ASM_Q8, TFA_IL_ASM_SRC4); }
          else if constexpr (PPW == 1) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P1_MF, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC1); }
          else { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P2_MF, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC2); }
        }
        else if constexpr (D == 128 && PPW == 2 && BF) { TFA_IL_ASM_LAZY_STMT(TFA_IL_ASM_LOOP); }
        else if constexpr (D == 128 && PPW == 2) { TFA_IL_ASM_LAZY_STMT(TFA_IL_ASM_LOOP_F16); }
        else if constexpr (D == 128 && BF) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D128_P4, TFA_IL_ASM_Q8, TFA_IL_ASM_SRC4); }
        else if constexpr (D == 128) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D128_P4_F16, TFA_IL_ASM_Q8, TFA_IL_ASM_SRC4); }
        else if constexpr (PPW == 1 && BF) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P1, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC1); }
        else if constexpr (PPW == 1) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P1_F16, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC1); }
        else if constexpr (BF) { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P2, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC2); }
        else { TFA_IL_ASM_LAZY_STMT_G(TFA_IL_ASM_LOOP_D64_P2_F16, TFA_IL_ASM_Q4, TFA_IL_ASM_SRC2); }
      }
    };
    auto asm_loop_exact = [&](int& j) {
      if constexpr (ASMLOOPX) {
        const int lim = fm < nact ? fm : nact;
        const int jend = (lim - 1 < nt_full - 2) ? lim - 1 : nt_full - 2;
        int koff = (j + 2) * k_tile_stride, voff = (j + 1) * v_tile_stride;
        const unsigned vaddr = lds_base + (unsigned)v_rd_base;
        const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds_base + wave * (PPW * 1024));
        float alpha;
        u32x4 f0, f1, f2, f3, ka;
        unsigned ka5, ka6, ka7;
        const int nact_s = __builtin_amdgcn_readfirstlane(nact), nt_s = __builtin_amdgcn_readfirstlane(nt);   // the tails' operands, as in asm_loop
        const int fmx = __builtin_amdgcn_readfirstlane(tail_on ? fm : -1);
        int ts;
        const int slim = __builtin_amdgcn_readfirstlane(wave_row0 + shift - key0_of(fm));
        if constexpr (std::is_same<T, __bf16>::value) { TFA_IL_ASM_EXACT_STMT(TFA_IL_ASM_LOOP_EXACT); }
        else { TFA_IL_ASM_EXACT_STMT(TFA_IL_ASM_LOOP_EXACT_F16); }
      }
    };
    if (!idle_wave)
#pragma nounroll
    for (int j = 0; j < nact; j += 2) {
      if constexpr (EXACT) {
        if (ASMLOOPX && (loop_ok(j) || tail_on)) {         // (the exact statement advances the maximum itself: it always makes progress)
          int jj = j;
          asm_loop_exact(jj);                          // tiles j .. jj-1 done, the running maximum advanced through tile jj-1
          if (jj & 1) j = jj - 1;
          else { j = jj - 2; continue; }
        } else
        if (j + 1 < nact) fast_exact(C0{}, j + 1 >= fm, j, sA, mA, sB, mB);
        else slow(j, sA, mA, sB, mB);
        if (j + 1 >= nact) break;
        if (j + 2 < nact) fast_exact(C1{}, j + 2 >= fm, j + 1, sB, mB, sA, mA);
        else slow(j + 1, sB, mB, sA, mA);
      } else {
      // (the statement makes progress from an even tile whenever no re-base is pending and either the loop proper takes the tile or the tails are on: then
      //  it runs to the wave's last tile and comes back early only for a re-base)
      if (ASMLOOP && !trigger(mA) && (loop_ok(j) || tail_on) && (!LOCAL || j + 1 >= nlm)) {
        int jj = j;
        asm_loop(jj, (early_ok && nact == nt) ? 1 : 0);   // tiles j .. jj-1 done, jj > j; S(jj) is in sA (jj even) / sB (odd)
#if defined(TFA_IL_TRACEITER)
        it_stamp(1 | (jj << 8));
#endif
        if (jj & 1) j = jj - 1;                        // on to the odd step below, for tile jj
        else { j = jj - 2; continue; }                 // back to the even step, for tile jj
      } else
      // (kernels that carry the statement keep NO compiler-scheduled pinned body: what the statement does not take — a tile with a re-base pending, the odd tile
      //  behind it, the last tiles of a block whose keys end inside a tile — goes to the burst-structured path, which serves any tile: same operations in the
      //  same order, bits identical; four unrolled instantiations of `fused` and their registers less in the kernel)
      if (!ASMLOOP && j + 1 < nact && !trigger(mA)) {
        if (SMOD ? !needs_mask(j + 1) : j + 1 < fm) fused(C0{}, MN{}, MN{}, 1.f, j, sA, sB, mB);   // (ALIBI, SOFTCAP: the pinned bodies take the left-edge tiles too)
        else fused(C0{}, MY{}, MN{}, 1.f, j, sA, sB, mB);
      } else {
        slow(j, sA, mA, sB, mB);
      }
      if (j + 1 >= nact) break;
      if (ASMLOOP && early_ok && nact == nt && j + 1 == nt - 1 && !trigger(mB)) {
        // the wave's last tile is the block's last (odd: nt is even): it runs in the block's last iteration below, behind the next pass's first requests
        last_pending = true;
        break;
      }
      if (!ASMLOOP && j + 2 < nact && !trigger(mB)) {
        if (SMOD ? !needs_mask(j + 2) : j + 2 < fm) fused(C1{}, MN{}, MN{}, 1.f, j + 1, sB, sA, mA);
        else fused(C1{}, MY{}, MN{}, 1.f, j + 1, sB, sA, mA);
      } else {
        slow(j + 1, sB, mB, sA, mA);
      }
      }
    }
#pragma nounroll
    for (int j = idle_wave ? 0 : (last_pending ? nt - 1 : nact); j < nt; ++j) {    // tiles of the block this wave does not touch (+ its own last one behind the early requests)
      if (early_ok && j == nt - 1) {                     // the block's last iteration: nothing of this pass left to ask for — the next pass's first requests, unwaited
        issue_early(block_of(pass + 1));
        early_done = true;
        if (last_pending) {
          int jj = j;
          asm_loop(jj, 2);                               // (odd entry -> dispatch -> the last-tile body without its vmcnt wait)
        } else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#if defined(TFA_IL_TRACEITER)
        it_stamp(2);
#endif
        break;
      }
      if (j + 2 < nt) dma_k(j + 2, j & 1);
      else if (seam) dma_k(j + 2 - nt, j & 1);
      if (j + 1 < nt) dma_v(j + 1, (j & 1) ^ 1);
      else if (seam) dma_v(0, (j & 1) ^ 1);
      iter_end();
    }
    // max-free rule: is every row sum still where the products P*v cannot have overflowed?  (this lane's half of its row; NaN fails the test too; the re-base
    // in rescale_if_needed sets the word as well when it meets such a sum in mid-pass.)  One LDS word, one barrier, every wave reads the same answer
    bool redo_pass = false;
    if constexpr (MAXFREE) {
      volatile int* const redo_w = reinterpret_cast<volatile int*>(smem + REDO_OFF);
      const float lt_ = (l4[0] + l4[1]) + (l4[2] + l4[3]);
      if (__any(!(lt_ <= 0x1p64f))) *redo_w = 1;
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      redo_pass = __builtin_amdgcn_readfirstlane(*redo_w) != 0 && !seeded;     // (a seeded pass has P <= 1: it is final whatever its sums are — inf in V, say)
      seeded = false;
    }
    if (P_TRACE && pass == tr_pass) t_loop = __builtin_amdgcn_s_memtime();
#if defined(TFA_IL_TRACEITER)
    if (P_TRACE && pass == tr_pass && blockIdx.x < 64) {      // the wave's records (16 x {cycle, tag}) out, behind the per-workgroup records
      typedef __attribute__((address_space(3))) const u32x2 lds_u32x2c;
      it_stamp(3 | (nt << 8) | (nact << 16));
      const int l_ = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
      if (l_ < 16) {
        const u32x2 r_ = *reinterpret_cast<lds_u32x2c*>(q_slice + l_ * 8);
        P_TRACE[(size_t)gridDim.x * 8 + ((size_t)blockIdx.x * 8 + wave_id) * 16 + l_] = l_ < it_n ? (((unsigned long long)r_[1] << 32) | r_[0]) : 0ull;
      }
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
#endif

