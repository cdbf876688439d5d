// tfa_fwd_il_epilogue.inc — per-pass epilogue of the issue-interleaved forward kernel: row sums, the key-split merge, LSE, O through LDS as whole rows
// A TEXTUAL piece of fwd_kernel_il (tfa_fwd_kernel_il.h includes it inside the kernel body, inside the pass loop): it is not a
// translation unit of its own and uses the kernel's locals.  Split out in round 3 without touching a token of the code — any edit
// here moves hipcc's schedule of the tile loop, so changes are judged by a same-process A/B (tools/ab_multi.py), never by eye.
    // ---- epilogue ---------------------------------------------------------------------------
    // every wave is past the last tile's barrier: the K/V buffers and qf are free -> ask for the next pass's first tiles
    // and Q now, so that their latency hides behind the normalisation and the stores below
    if (PREF && !PREF2 && more_passes) issue_prologue(next_mb, true);
    if (SEAM) { seam_in = seam; if (seam) issue_prologue(next_mb, false); }   // Q only: K(0), K(1), V(0) are on chip
    // (the lane's coordinates are RE-DERIVED here — v_mbcnt, two instructions — instead of carried from the kernel's start: the start-up values otherwise
    //  stay live across the tile loop for the epilogue's sake alone, and the loop has no register to spare; round 5)
    // (round 6: the kernel arguments the epilogue needs are read AGAIN from the kernarg segment, through a pointer the compiler cannot see through — as values
    //  of `p` they stay live in SGPRs from the kernel's first instruction across every tile loop, and with ~100 scalars live hipcc parks them in lanes of a
    //  VGPR: the epilogue then fetched them back one v_readlane + s_nop at a time — 26 of them, 62 once the max-free rule added a few more long-lived scalars)
    typedef __attribute__((address_space(4))) const KArgs kargs_c;
    kargs_c* pe_ = (kargs_c*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pe_));
    kargs_c& pe = *pe_;
    VarSeq vse{};                                      // VARLEN: the sequence's rows re-read with the arguments; its LSE row is h * total_q + q0 + row
    if constexpr (VARLEN) vse = varlen_seq(pe, b);
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int qi_e = lane_e & 31, hi_e = lane_e >> 5, my_row_e = wave_row0 + qi_e;
    float l_tot = pair_sum((l4[0] + l4[1]) + (l4[2] + l4[3]));
    float w0 = 1.f, w1 = 0.f;                          // KSPLIT: weights of this group's and the other group's partial result
    const char* const dump = smem + 4 * TILE_BYTES;    // KSPLIT: group 1's (now idle) tile buffers carry its O to group 0
    if constexpr (KSPLIT) {
      // the two groups hold partial results over disjoint key sets: group 1 writes (m, l, O) — lane-private data, no
      // transposition — and leaves; group 0 merges by the split-KV rule (tfa_merge.hip) while it reads its own O out
      float* const ml = reinterpret_cast<float*>(smem + wave * (32 * D * 2)) + lane_e * 2;   // (in group 0's idle buffers)
      if (grp == 1) {
        ml[0] = mref; ml[1] = l_tot;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          float o[16];
          if (d == 0) o_read<0>(o, 1.f); else if (d == 1) o_read<1>(o, 1.f); else if (d == 2) o_read<2>(o, 1.f); else o_read<3>(o, 1.f);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 v4 = {o[4 * g + 0], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
            *reinterpret_cast<f32x4*>(const_cast<char*>(dump) + ((((wave * DT + d) << 2) + g) << 10) + lane_e * 16) = v4;
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (grp == 1) {
        if (!more_passes) return;
        // paired causal blocks: group 0 still reads this group's buffers (the dump) and writes its own (epilogue slices);
        // the next pass's first DMA pieces wait behind the barrier group 0 ends its epilogue with
        asm volatile("s_barrier" ::: "memory");
        continue;
      }
      const float m1 = ml[0], l1 = ml[1];
      const float m = fmaxf(mref, m1);
      w0 = (mref == -INFINITY) ? 0.f : fast_exp2(mref - m);
      w1 = (m1 == -INFINITY) ? 0.f : fast_exp2(m1 - m);
      l_tot = w0 * l_tot + w1 * l1;
      mref = m;
    }
    const bool empty = !(l_tot > 0.f);
    const float inv = empty ? 1.f : 1.f / l_tot;
    // O[d tile d][0..15] of this lane, normalised (KSPLIT: merged with the other group's)
    auto o_get = [&](int d, float (&o)[16]) {
      const float f0 = inv * w0;
      if (d == 0) o_read<0>(o, f0); else if (d == 1) o_read<1>(o, f0); else if (d == 2) o_read<2>(o, f0); else o_read<3>(o, f0);
      if constexpr (KSPLIT) {
        const float f1 = inv * w1;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(dump + ((((wave * DT + d) << 2) + g) << 10) + lane_e * 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[4 * g + e] = fmaf(f1, x[e], o[4 * g + e]);
        }
      }
    };
    if (PREF2) {
      // ONE store instruction per wave, always issued (the early requests of a pair's second pass are older than it: the counted vmcnt below relies on the
      // count): through a descriptor of this head's LSE row — rows beyond Nq, the second half-wave and a null pointer are out of its range and dropped
      const float lse = empty ? INFINITY : (mref + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
      auto lse_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(VARLEN ? pe.lse + ((long long)h * pe.total_q + vse.q0) : pe.lse + (long long)bh * pe.Nq), 0,
                                                      pe.lse != nullptr ? (unsigned)(VARLEN ? vse.nq : pe.Nq) * 4u : 0u, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, lse), lse_rs, hi_e == 0 ? my_row_e * 4 : (int)TFA_OOB, 0, 0);
    } else
    if (pe.lse != nullptr && hi_e == 0 && my_row_e < (VARLEN ? vse.nq : pe.Nq)) {
      const float lse = empty ? INFINITY : (mref + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
      if constexpr (VARLEN) pe.lse[(long long)h * pe.total_q + vse.q0 + my_row_e] = lse;
      else pe.lse[(long long)bh * pe.Nq + my_row_e] = lse;
    }
    if (PREF2 && more_passes && !early_done) {
      // behind the LSE store, in front of the O stores: exactly NST_EPI vector-memory instructions follow these requests
      asm volatile("" ::: "memory");
      issue_prologue(next_mb, true);
      asm volatile("" ::: "memory");
    }
    if (F32OUT) {
      float* obase = reinterpret_cast<float*>(pe.o) + (VARLEN ? (long long)vse.q0 * pe.os_n : b * pe.os_b) + h * pe.os_h;
      auto o_rs = slice_rsrc(obase, VARLEN ? varlen_bytes(vse.nq, pe.os_n, pe.dv, 4) : pe.o_bytes, (unsigned long long)q0 * (unsigned long long)pe.os_n * 4ull);
      const int ooff = (my_row_e - (WIN ? q0 : 0)) * (int)pe.os_n * 4 + hi_e * 16;
      // (PREF2's counted wait below relies on EXACTLY NST_EPI vector-memory instructions behind the next pass's requests: every store is issued —
      //  chunks beyond dv and rows beyond Nq go out of range, never skipped — and the trip counts are pinned to the constant here)
      static_assert(!F32OUT || NST_EPI == DT * 4, "NST_EPI must equal the fp32 epilogue's store count");
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        float o[16];
        o_get(d, o);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v4 = {o[4 * g + 0], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v4), o_rs, d * 32 + g * 8 + hi_e * 4 < pe.dv ? ooff + (d * 32 + g * 8) * 4 : (int)TFA_OOB, 0, 0);
        }
      }
    } else if (EPI) {
      // A lane holds 4-element pieces of ONE row spread over 16 register groups: stored directly that is 16 eight-byte
      // stores per lane, 32 different rows per instruction.  Instead the wave transposes its 32 x D tile through its own
      // slice of the epilogue region (16-byte chunk index XOR row, as for K) and writes whole rows: 1 KiB contiguous per
      // store instruction.  The region is separate from the tile buffers (which the next pass is already filling).
      T* obase = reinterpret_cast<T*>(pe.o) + (VARLEN ? (long long)vse.q0 * pe.os_n : b * pe.os_b) + h * pe.os_h;
      auto o_rs = slice_rsrc(obase, VARLEN ? varlen_bytes(vse.nq, pe.os_n, pe.dv, 2) : pe.o_bytes, (unsigned long long)q0 * (unsigned long long)pe.os_n * 2ull);
      typedef __attribute__((ext_vector_type(4))) T t4;
      // (the lane ids go through an empty asm so that none of the 24 addresses below is loop-invariant: hoisted out of
      // the pass loop they would stay live across the main loop and spill)
      int qix = qi_e, lanex = lane_e;
      asm volatile("" : "+v"(qix), "+v"(lanex));
      constexpr bool INPLACE = (VF & VF_IL_EPI_INPLACE) != 0;
      static_assert(!INPLACE || !PREF, "in-place epilogue slices would be overwritten by the next pass's prefetch");
      char* const ow = smem + (INPLACE ? 0 : 4 * TILE_BYTES) + wave * (32 * D * 2);
      constexpr int CH = D / 8;                      // 16-byte chunks per row
      const int osw = (CH == 16) ? (qix & 15) : (qix & 7);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        float o[16];
        o_get(d, o);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          t4 v4 = {(T)o[4 * g + 0], (T)o[4 * g + 1], (T)o[4 * g + 2], (T)o[4 * g + 3]};
          const int c = d * 4 + g;
          *reinterpret_cast<u32x2*>(ow + qix * (D * 2) + ((c ^ osw) << 4) + (lanex >> 5) * 8) = __builtin_bit_cast(u32x2, v4);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private slice: no barrier needed
      constexpr int RPI = 64 / CH;                   // rows per store instruction (4 at D=128, 8 at D=64)
      static_assert(F32OUT || NST_EPI == 32 / RPI, "NST_EPI must equal the row-store count of the LDS epilogue (PREF2's counted vmcnt)");
#pragma unroll
      for (int i = 0; i < 32 / RPI; ++i) {
        const int r = i * RPI + lanex / CH, cpos = lanex % CH;
        const int c = cpos ^ ((CH == 16) ? (r & 15) : (r & 7));
        u32x4 v = *reinterpret_cast<const u32x4*>(ow + r * (D * 2) + (cpos << 4));
        __builtin_amdgcn_raw_buffer_store_b128(v, o_rs, c * 8 < pe.dv ? (wave_row0 - (WIN ? q0 : 0) + r) * (int)pe.os_n * 2 + (c << 4) : (int)TFA_OOB, 0, IL_OSTORE_AUX);
      }
      if (INPLACE) {
        // the next pass's first DMA pieces land in these buffers: every wave must have read its rows back
        if (!KSPLIT && more_passes) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // (KSPLIT: below, every output type)
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slice is rewritten by this wave's next epilogue only
      }
    } else {
      T* obase = reinterpret_cast<T*>(pe.o) + (VARLEN ? (long long)vse.q0 * pe.os_n : b * pe.os_b) + h * pe.os_h;
      auto o_rs = slice_rsrc(obase, VARLEN ? varlen_bytes(vse.nq, pe.os_n, pe.dv, 2) : pe.o_bytes, (unsigned long long)q0 * (unsigned long long)pe.os_n * 2ull);
      const int ooff = (my_row_e - (WIN ? q0 : 0)) * (int)pe.os_n * 2 + hi_e * 8;
      typedef __attribute__((ext_vector_type(4))) T t4;
      static_assert(F32OUT || EPI || NST_EPI == DT * 4, "NST_EPI must equal the direct 16-bit epilogue's store count");
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        float o[16];
        o_get(d, o);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          t4 v4 = {(T)o[4 * g + 0], (T)o[4 * g + 1], (T)o[4 * g + 2], (T)o[4 * g + 3]};
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v4), o_rs, d * 32 + g * 8 + hi_e * 4 < pe.dv ? ooff + (d * 32 + g * 8) * 2 : (int)TFA_OOB, 0, 0);
        }
      }
    }
    if (PREF2) {
      // (unconditional: on the last pass nothing was requested and nothing is waited for, but a wait under the same condition as the
      //  requests is a second branch, and hipcc's model then sees a path "requested, not waited" into the loop header.)
      // vmcnt retires in issue order and exactly NST_EPI store instructions follow the next pass's requests: once at most that many
      // operations are outstanding, K(0), V(0), K(1) are in LDS and Q in registers, while the O stores (a write acknowledge under the
      // whole chip's store burst) stay in flight.  Here, not in the next prologue: hipcc's own wait for the Q registers is exact in
      // this straight-line code (vmcnt(NST_EPI)), but vmcnt(0) behind the loop's back edge, where it merges with the first pass
      if (more_passes) o_zero<DT>();              // the next pass's accumulators, in front of the wait for its operands
      if (early_done) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST_EPI + 1) : "memory");   // (early requests: the LSE store is younger than they are, too)
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST_EPI) : "memory");
#pragma unroll
      for (int s = 0; s < DS; ++s) asm volatile("" : "+v"(qf[s]));
    }
    // KSPLIT, another pass to come: group 0 has read group 1's dump and its own epilogue slices — both live in tile buffers the
    // next pass's first DMA pieces overwrite (group 1 waits at the matching barrier right behind the merge)
    if (KSPLIT && more_passes) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
