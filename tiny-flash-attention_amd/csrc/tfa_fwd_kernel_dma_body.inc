// tfa_fwd_kernel_dma_body.inc — the body of the LDS-DMA forward kernel (tfa_fwd_kernel_dma.h), included inside its two __global__ entry points.  In scope: the kernel
// argument `p` (KArgs, or KvcArgs in the KV-cache form) and T, D, NW, CAUSAL, F32OUT, VF, AB.
  using E = Elem<T>;
  constexpr bool KVC = (VF & VF_KVCACHE) != 0;
  constexpr bool KV8 = (VF & VF_KV_E4M3) != 0;     // the K/V cache holds e4m3 bytes (tfa_fwd_kvcache_fp8): tiles are staged through registers and decoded to T on the way into LDS
  // the packed form of the KV-cache form (KvcPacked: GQA query heads as position-major rows, row = t * G + g); its arguments are read through KvcPackView<PACK>::of(p),
  // a dependent expression every other entry point never instantiates
  constexpr bool PACK = KVC && KvcPack<decltype(p)>::value;
  // the varlen-q form of the KV-cache form (KvcVarlenQ: packed ragged query rows, every sequence's first row and row count read on the device); its arguments are read
  // through KvcVqView<VQ>::of(p), as above
  constexpr bool VQ = KVC && KvcVq<decltype(p)>::value;
  // the scheduled form of the varlen-q form (KvcSched: the work items of a device-built list); its arguments are read through KvcScView<SCHED>::of(p), as above
  constexpr bool SCHED = VQ && KvcSc<decltype(p)>::value;
  // the windowed form of any of those (KvcWindow: a sliding window of win_left keys in front of a row's own); its argument is read through KvcWinView<WIN>::of(p), as above
  constexpr bool WIN = KVC && KvcWin<decltype(p)>::value;
  // the tree form of any of the KV-cache forms (KvcTree: one 64-bit visibility word per query row over the step's new keys); its arguments are read through
  // KvcTreeView<TREE>::of(p), as above
  constexpr bool TREE = KVC && KvcTr<decltype(p)>::value;
  constexpr int ES = KV8 ? 1 : 2;                  // bytes per K/V element in memory
  using KT = typename KvElem<KV8, T>::type;
  using X8 = typename E::x8;
  constexpr int BM = NW * 32;
  constexpr int BN = 64;
  constexpr int CPR = D / 8;                       // 16-byte chunks per row
  constexpr int TILE_BYTES = BN * D * 2;           // one K (or V) tile
  constexpr int NBUF = (VF & VF_2BUF) ? 2 : 3;     // LDS tile buffers; tiles 0..NBUF-2 ahead are in flight
  constexpr int PD = NBUF - 1;                     // prefetch distance in tiles
  constexpr int PIECES = TILE_BYTES / 1024;        // 1 KiB DMA pieces per tensor per tile
  constexpr int PPW = PIECES / NW;                 // pieces per wave per tensor
  constexpr int DS = D / 16;
  constexpr int DT = D / 32;
  constexpr bool PAIR = CAUSAL && (VF & VF_PAIR);
  constexpr bool WIDE = D > 128;
  static_assert(PPW >= 1 && PPW * NW == PIECES, "tile does not split into whole DMA pieces per wave");
  static_assert(!WIDE || (NW == 4 && AB == 0), "the 256-wide form: four waves, no ablations");
  static_assert(!KVC || (!WIDE && AB == 0 && !(VF & (VF_PERSIST | VF_LDSEPI))), "the KV-cache form: 64 / 128 wide, one work item per workgroup");
  static_assert(!SCHED || !(VF & VF_PERSIST), "the scheduled form: one work item per workgroup (an item behind the list's end returns)");
  static_assert(!WIN || (CAUSAL && PAIR), "the windowed form: a form of the causal KV-cache kernel");
  static_assert(!TREE || (CAUSAL && PAIR && !WIN), "the tree form: a form of the causal KV-cache kernel, without a window");
  static_assert(!KV8 || (KVC && NBUF == 2), "the e4m3 form: a form of the two-buffer KV-cache kernel (one tile staged in registers)");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const kl = smem;                           // K buffers 0..2
  char* const vl = smem + NBUF * TILE_BYTES;       // V buffers 0..2
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  unsigned long long t_start = 0, t_pro = 0, t_loop = 0, rt_start = 0;
  if (p.trace) { rt_start = __builtin_amdgcn_s_memrealtime(); t_start = __builtin_amdgcn_s_memtime(); }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 31;
  const int hi = lane >> 5;
  // split-KV in ONE launch (tfa_fwd_splitkv): the grid carries nsplit copies of the work items; copy sp handles the key
  // chunk [sp*chunk, sp*chunk + nk) with the causal shift reduced by the chunk offset and writes its fp32 partial O and
  // LSE at sp * part stride.  nsplit <= 1: one chunk = the whole K/V tensor.
  const int nsplit = p.nsplit > 1 ? p.nsplit : 1;
  const int nitems0 = p.nbh * p.nwork;
  const int nitems = nitems0 * nsplit;

  // ---- per-lane DMA source offsets (tile 0); the LDS destination of piece pc is pc*1024 + lane*16
  int k_src[PPW], v_src[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int pc = wave * PPW + i;
    {  // K: row-major, chunk position c' holds source chunk c' ^ swz(row)
      const int row = pc * (1024 / (D * 2)) + lane / CPR;
      const int cpos = lane % CPR;
      const int kch = cpos ^ k_swz<D>(row);            // source chunk of this lane; chunks beyond the valid head dim read as zeros
      k_src[i] = kch * 8 < p.dv ? row * (int)p.ks_n * ES + kch * (8 * ES) : (int)TFA_OOB;
    }
    {  // V: invert v_lds_off(): LDS offset -> (key, 16-byte chunk)
      const int o = pc * 1024 + lane * 16;
      const int sub = o >> 9, R = (o >> 6) & 7, pcs = (o >> 4) & 3;
      const int dt = sub % DT, sh = sub / DT;
      const int key = 16 * (sh >> 1) + 4 * (sh & 1) + 8 * (R >> 2) + (R & 3);
      v_src[i] = (dt * 4 + pcs) * 8 < p.dv ? key * (int)p.vs_n * ES + (dt * 4 + pcs) * (8 * ES) : (int)TFA_OOB;
    }
  }
  const int k_tile_stride = BN * (int)p.ks_n * ES;
  const int v_tile_stride = BN * (int)p.vs_n * ES;

  const int k_rd_base = qi * (D * 2);
  const int k_rd_swz = k_swz<D>(qi);
  const int i16 = lane & 15, g16 = (lane >> 4) & 1;
  const int v_rd_base = (hi * DT << 9) + ((i16 >> 2) << 6) + (g16 << 5) + ((i16 & 3) << 3);
  float sc = p.scale_log2;
  // e4m3 form: the descales of the work item's (sequence, K/V head) — k_descale goes into the score scale (sc, and the LSE's), v_descale into the epilogue.  One
  // decode() reads them for the block it describes; the epilogue of the block before uses the copies taken in front of that decode() (cur_scale_lse, cur_vd)
  float scale_lse = p.scale, vd_w = 1.f;
  u32x2 st_k[KV8 ? PPW : 1], st_v[KV8 ? PPW : 1];   // e4m3 form: the tile in flight (8 bytes per piece and tensor)

  // ---- the block stream ----------------------------------------------------------------------
  struct Blk {
    int bh, wi, mb, nt;
    int sp, nk, shift;          // key chunk index, keys in the chunk, causal shift against the chunk's local key index
    __amdgpu_buffer_rsrc_t q_rs, k_rs, v_rs;
    // KV-cache form, paged: first 64-key tile of the chunk (global tile index), the sequence's row of the block table, the K/V head's offset inside a page
    int tile0, bt_row;
    long long k_hoff, v_hoff;
  };
  // paged: the block-table entry of the page the last tile issued lies in — one scalar load per page, not per tile (tiles are issued in ascending order; the
  // entry of the NEXT tile's page is requested right behind a tile's DMA pieces, a tile of compute ahead of its use)
  int pg_idx = -1, pg_val = 0;
  // varlen-q form: the first query row, the row count and the block rows (nq_b * G packed) of the sequence the last decode() described
  int vq_q0 = 0, vq_nq = 0, vq_rows = 0;
  // scheduled form: the item's index among its sequence's own items, that sequence's block count (>= 1), and whether the index lies behind the list's end
  int sc_wi = 0, sc_nmb = 1;
  bool sc_dead = false;
  auto decode = [&](int item_all, int pass, Blk& k) {
    k.sp = item_all / nitems0;
    const int item = item_all - k.sp * nitems0;
    k.nk = p.Nk;
    k.shift = p.shift;
    if constexpr (KVC) {
      const KvcArgs& pk = KvcView<KVC>::of(p);
      // the sequence's length, read by the work item itself (b is wave-uniform: a scalar load, as the varlen kernels read cu_seqlens) and clamped into the
      // cache; the chunk size comes from THIS sequence's length, so ragged batches stay balanced; a chunk behind the end is empty (nt = 0: out = 0, lse = +inf)
      typedef __attribute__((address_space(4))) const int cint4;
      const int bh0 = ((p.nbh & 7) == 0) ? (item & 7) + 8 * ((item >> 3) / p.nwork) : item / p.nwork;
      int b0 = bh0 / p.H;
      if constexpr (SCHED) {
        // nbh = heads and nwork = bound: bh0 is the head, the index inside the head the row of the list.  n_items and the row are one scalar load each; both are
        // hints — n_items clamped into [0, bound] (the rows the buffer holds), b into [0, B), wi checked against the sequence's own items below
        const auto& ps = KvcScView<SCHED>::of(p);
        typedef __attribute__((ext_vector_type(2))) int i32x2;
        typedef __attribute__((address_space(4))) const i32x2 ci32x2;
        const int si = ((p.nbh & 7) == 0) ? (item >> 3) % p.nwork : item % p.nwork;
        int n_items = ((const cint4*)(uintptr_t)ps.sc_meta)[0];
        n_items = n_items < 0 ? 0 : (n_items > ps.sc_bound ? ps.sc_bound : n_items);
        sc_dead = si >= n_items;
        i32x2 row = {0, -1};
        if (!sc_dead) row = ((ci32x2*)(uintptr_t)ps.sc_meta)[SCHED_HDR / 2 + si];
        b0 = row[0] < 0 ? 0 : (row[0] >= p.B ? p.B - 1 : row[0]);
        sc_wi = row[1];
      }
      int len = ((const cint4*)(uintptr_t)pk.seqlens)[b0] + pk.n_new;
      len = len < 0 ? 0 : (len > pk.capacity ? pk.capacity : len);
      int chunk = (fd_div(len + nsplit - 1, pk.fd_nsplit) + 63) & ~63;
      int rest = len - k.sp * chunk;
      k.nk = rest < chunk ? (rest > 0 ? rest : 0) : chunk;
      int nq_pos = pk.nq_pos;
      if constexpr (VQ) {
        // the sequence's rows of the packed q, read and clamped as the length is: whatever cu_seqlens_q holds, [q0, q0 + nq) lies inside [0, total_q) and nq <= max_q
        const auto& pv = KvcVqView<VQ>::of(p);
        const int c0 = ((const cint4*)(uintptr_t)pv.vq_cu)[b0], c1 = ((const cint4*)(uintptr_t)pv.vq_cu)[b0 + 1];
        vq_q0 = c0 < 0 ? 0 : (c0 > pv.vq_total_q ? pv.vq_total_q : c0);
        const int room = pv.vq_total_q - vq_q0 < pv.vq_max_q ? pv.vq_total_q - vq_q0 : pv.vq_max_q;
        const long long d = (long long)c1 - c0;
        vq_nq = d < 0 ? 0 : (d > room ? room : (int)d);
        vq_rows = vq_nq;
        if constexpr (PACK) vq_rows = vq_nq * KvcPackView<PACK>::of(p).pk_g;
        if constexpr (SCHED) {
          // the sequence's own blocks and items, from the rows just clamped; a wi that is none of them is an item of a sequence without rows (nothing requested or stored)
          sc_nmb = (vq_rows + BM - 1) / BM;
          const int items_b = PAIR ? (sc_nmb + 1) >> 1 : sc_nmb;
          if (sc_wi < 0 || sc_wi >= items_b) { vq_nq = 0; vq_rows = 0; sc_wi = 0; sc_nmb = 1; }
        }
        nq_pos = vq_nq;
      }
      k.shift = len - nq_pos - k.sp * chunk;
      k.tile0 = (k.sp * chunk) >> 6;
      if constexpr (WIN) {
        // the chunks are cut from [lo64, len): lo the first key the sequence's first row sees, rounded down to a tile; shift counts against the chunk's first key
        const int lo = len - nq_pos - KvcWinView<WIN>::of(p).win_left;
        const int lo64 = lo > 0 ? lo & ~63 : 0;
        chunk = (fd_div(len - lo64 + nsplit - 1, pk.fd_nsplit) + 63) & ~63;
        rest = len - lo64 - k.sp * chunk;
        k.nk = rest < chunk ? (rest > 0 ? rest : 0) : chunk;
        k.shift = len - nq_pos - lo64 - k.sp * chunk;
        k.tile0 = (lo64 + k.sp * chunk) >> 6;
      }
      k.bt_row = b0;
      pg_idx = -1;
    } else if (nsplit > 1) {
      const int rest = p.Nk - k.sp * p.chunk;
      k.nk = rest < p.chunk ? (rest > 0 ? rest : 0) : p.chunk;
      k.shift = p.shift - k.sp * p.chunk;
    }
    if ((p.nbh & 7) == 0) {          // heads of one XCD stay together (item & 7 == blockIdx & 7 when G % 8 == 0)
      const int x = item & 7, s = item >> 3;
      k.bh = x + 8 * (s / p.nwork);
      k.wi = s % p.nwork;
    } else {
      k.bh = item / p.nwork;
      k.wi = item % p.nwork;
    }
    int nmb = p.nmb;
    if constexpr (SCHED) {                                       // the list's (sequence, item) and the sequence's own block count in the place of the launch's
      k.bh = k.bt_row * p.H + k.bh;
      k.wi = sc_wi;
      nmb = sc_nmb;
    }
    if (PAIR) k.mb = pass == 0 ? (nmb - 1 - k.wi) : k.wi;       // heavy block first, then the light one
    else k.mb = CAUSAL ? (nmb - 1 - k.wi) : k.wi;
    if constexpr (WIN) {
      // the block's first tile: the first one the block's first row (packed: its position) sees.  The chunk is narrowed to start there — tile0, shift and nk move
      // together — so tile 0 of everything below (the two prefetched tiles, the loop, the buffer rotation, the contiguous descriptors' base) is that tile
      int t_first = k.mb * BM;
      if constexpr (PACK) t_first = fd_div(t_first, KvcPackView<PACK>::of(p).pk_fd_g);
      const int c = t_first + k.shift - KvcWinView<WIN>::of(p).win_left;
      const int j0 = c > 0 ? c >> 6 : 0;
      k.tile0 += j0;
      k.shift -= j0 * BN;
      k.nk = k.nk > j0 * BN ? k.nk - j0 * BN : 0;
    }
    int kv_end = k.nk;
    if (CAUSAL) {
      int lim = k.mb * BM + BM + k.shift;                        // one past the last key any row of the block sees
      if constexpr (PACK) {                                      // ... the position of the block's last valid row sees
        int rows = p.Nq;
        if constexpr (VQ) rows = vq_rows > 0 ? vq_rows : 1;      // (a sequence without rows: every block of it is empty, below)
        const int last = k.mb * BM + BM - 1 < rows - 1 ? k.mb * BM + BM - 1 : rows - 1;
        lim = fd_div(last, KvcPackView<PACK>::of(p).pk_fd_g) + 1 + k.shift;
      }
      kv_end = lim < kv_end ? lim : kv_end;
    }
    k.nt = kv_end > 0 ? (kv_end + BN - 1) / BN : 0;
    if constexpr (VQ) {
      if (k.mb * BM >= vq_rows) k.nt = 0;                        // a block without rows of its sequence: no K/V tile (prefetch: no Q either; the epilogue: no store)
    }
    const int b = k.bh / p.H, h = k.bh - b * p.H, hk = h / (p.H / p.Hk);
    const T* q_base = reinterpret_cast<const T*>(p.q) + b * p.qs_b + h * p.qs_h;
    unsigned q_ext = (unsigned)p.q_bytes;
    if constexpr (VQ) {                                          // from the sequence's first row to its last (qs_b is 0; the host bounds max_q rows by 2 GiB)
      long long e = (long long)(vq_nq - 1) * p.qs_n + p.dv;
      if constexpr (PACK) e += (long long)(KvcPackView<PACK>::of(p).pk_g - 1) * KvcPackView<PACK>::of(p).q_hs;
      q_base += (long long)vq_q0 * p.qs_n;
      q_ext = vq_nq > 0 ? (unsigned)(e * 2) : 0u;
    }
    k.q_rs = __builtin_amdgcn_make_buffer_rsrc((void*)q_base, 0, q_ext, 0x00020000);
    unsigned kb = (unsigned)p.k_bytes, vb = (unsigned)p.v_bytes;
    long long koff = 0, voff = 0;
    if constexpr (KVC) {
      const KvcArgs& pk = KvcView<KVC>::of(p);
      // as below, for every split count: the extent ends at the last valid key of the chunk, so whatever the cache holds behind the sequence's length — the
      // tail of a page, stale keys of an earlier request, NaN — reads as zeros.  Paged: per-tile descriptors (dma_issue), these two stay empty
      if (pk.block_table != nullptr) {
        k.k_hoff = (long long)hk * p.ks_h;
        k.v_hoff = (long long)hk * p.vs_h;
        kb = vb = 0u;
      } else {
        koff = (long long)k.tile0 * 64 * p.ks_n;
        voff = (long long)k.tile0 * 64 * p.vs_n;
        kb = k.nk > 0 ? (unsigned)(((long long)(k.nk - 1) * p.ks_n + p.dv) * ES) : 0u;
        vb = k.nk > 0 ? (unsigned)(((long long)(k.nk - 1) * p.vs_n + p.dv) * ES) : 0u;
      }
    } else if (nsplit > 1) {                                     // descriptor over the chunk only: OOB rows read as zeros
      koff = (long long)k.sp * p.chunk * p.ks_n;
      voff = (long long)k.sp * p.chunk * p.vs_n;
      // (extent of nk rows of the VALID width p.dv: with the kernel's width D here, a head dim below D would leave the first
      //  row behind the chunk readable — for the last chunk of the last head that is memory behind the tensor, and P = 0
      //  times whatever lies there is NaN as soon as it is not finite; found by tools/fuzz_fwd.py --decode)
      kb = k.nk > 0 ? (unsigned)(((long long)(k.nk - 1) * p.ks_n + p.dv) * 2) : 0u;
      vb = k.nk > 0 ? (unsigned)(((long long)(k.nk - 1) * p.vs_n + p.dv) * 2) : 0u;
    }
    k.k_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const KT*>(p.k) + b * p.ks_b + hk * p.ks_h + koff), 0, kb, 0x00020000);
    k.v_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const KT*>(p.v) + b * p.vs_b + hk * p.vs_h + voff), 0, vb, 0x00020000);
    if constexpr (KV8) {
      const Kvc8Args& p8 = Kvc8View<KV8>::of(p);
      typedef __attribute__((address_space(4))) const float cfloat4;
      const float kd = p8.k_descale ? ((cfloat4*)(uintptr_t)p8.k_descale)[b * p8.kd_b + hk * p8.kd_h] : 1.f;
      vd_w = p8.v_descale ? ((cfloat4*)(uintptr_t)p8.v_descale)[b * p8.vd_b + hk * p8.vd_h] : 1.f;
      sc = p.scale_log2 * kd;
      scale_lse = p.scale * kd;
    }
  };
  // KV-cache form, paged: the page of global tile `gt` of block-table row `row` (clamped into the cache: a bad entry can misplace a read, never leave the tensors)
  auto page_of = [&](int row, int gt) -> int {
    if constexpr (KVC) {
      const KvcArgs& pk = KvcView<KVC>::of(p);
      typedef __attribute__((address_space(4))) const int cint4;
      const int pidx = fd_div(gt, pk.fd_tpp);
      if (pidx != pg_idx) {
        pg_idx = pidx;
        const int v = ((const cint4*)(uintptr_t)pk.block_table)[(long long)row * pk.bt_stride + pidx];
        pg_val = v < 0 ? 0 : (v >= pk.num_pages ? pk.num_pages - 1 : v);
      }
    }
    return pg_val;
  };
  // VF_DMA_NT: every K/V byte is read by exactly one workgroup (one query block per head, GQA rows packed) AND the cache is larger
  // than the 256 MB memory-side cache can keep from one decode step to the next (the host decides: tfa_api.hip) -> non-temporal
  // loads: +8..16 % on caches of 1 GB; caches that fit are served faster without the hint (-15 %: profiles/r03_decode_nt_ab.txt)
  auto dma_issue = [&](const Blk& k, int j, int buf) {
    if constexpr (KVC) {
      const KvcArgs& pk = KvcView<KVC>::of(p);
      if (pk.block_table != nullptr) {
        // one descriptor per 64-key tile (a tile never straddles pages: page_size is a multiple of 64): base = the tile's first row inside its page, extent = up
        // to the last valid key.  lds_dma16's s_nop 4 covers "SALU wrote the descriptor -> VMEM reads it" (the pattern of lds_dma16_m0_fresh)
        const int gt = k.tile0 + j;
        const int pidx = fd_div(gt, pk.fd_tpp);
        const long long page = page_of(k.bt_row, gt);
        const int row0 = (gt - pidx * pk.tpp) << 6;
        int rows = k.nk - j * BN;
        rows = rows > BN ? BN : rows;
        const unsigned kb = rows > 0 ? (unsigned)(((long long)(rows - 1) * p.ks_n + p.dv) * ES) : 0u;
        const unsigned vb = rows > 0 ? (unsigned)(((long long)(rows - 1) * p.vs_n + p.dv) * ES) : 0u;
        const auto k_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const KT*>(p.k) + page * p.ks_b + k.k_hoff + (long long)row0 * p.ks_n), 0, kb, 0x00020000);
        const auto v_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const KT*>(p.v) + page * p.vs_b + k.v_hoff + (long long)row0 * p.vs_n), 0, vb, 0x00020000);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
          const int pc = wave * PPW + i;
          if constexpr (KV8) {
            st_k[i] = kv8_load<(VF & VF_DMA_NT) != 0>(k_rs, k_src[i]);
            st_v[i] = kv8_load<(VF & VF_DMA_NT) != 0>(v_rs, v_src[i]);
          } else if constexpr ((VF & VF_DMA_NT) != 0) {
            lds_dma16_nt(k_rs, lds_base + buf * TILE_BYTES + pc * 1024, k_src[i]);
            lds_dma16_nt(v_rs, lds_base + (NBUF + buf) * TILE_BYTES + pc * 1024, v_src[i]);
          } else {
            lds_dma16(k_rs, lds_base + buf * TILE_BYTES + pc * 1024, k_src[i]);
            lds_dma16(v_rs, lds_base + (NBUF + buf) * TILE_BYTES + pc * 1024, v_src[i]);
          }
        }
        if ((j + 1) * BN < k.nk) (void)page_of(k.bt_row, gt + 1);     // the next tile's page, requested a tile ahead
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int pc = wave * PPW + i;
      if constexpr (KV8) {
        st_k[i] = kv8_load<(VF & VF_DMA_NT) != 0>(k.k_rs, k_src[i] + j * k_tile_stride);
        st_v[i] = kv8_load<(VF & VF_DMA_NT) != 0>(k.v_rs, v_src[i] + j * v_tile_stride);
      } else if constexpr ((VF & VF_DMA_NT) != 0) {
        lds_dma16_nt(k.k_rs, lds_base + buf * TILE_BYTES + pc * 1024, k_src[i] + j * k_tile_stride);
        lds_dma16_nt(k.v_rs, lds_base + (NBUF + buf) * TILE_BYTES + pc * 1024, v_src[i] + j * v_tile_stride);
      } else {
        lds_dma16(k.k_rs, lds_base + buf * TILE_BYTES + pc * 1024, k_src[i] + j * k_tile_stride);
        lds_dma16(k.v_rs, lds_base + (NBUF + buf) * TILE_BYTES + pc * 1024, v_src[i] + j * v_tile_stride);
      }
    }
  };
  // e4m3 form: the staged tile, decoded (exactly: every e4m3 value is a T) and written to the 16 LDS bytes per piece this lane's DMA would have filled
  auto stage_commit = [&](int buf) {
    if constexpr (KV8) {
#pragma unroll
      for (int i = 0; i < PPW; ++i) {
        const int o = (wave * PPW + i) * 1024 + lane * 16;
        lds_write_b128(kl, buf * TILE_BYTES + o, kv8_decode<T>(st_k[i]));
        lds_write_b128(vl, buf * TILE_BYTES + o, kv8_decode<T>(st_v[i]));
      }
    }
  };
  X8 qf[DS];
  // request a block's first two K/V tiles and its Q fragments (nothing is waited for here)
  auto prefetch = [&](const Blk& k) {
    if (k.nt > 0) dma_issue(k, 0, 0);
    if (PD > 1 && k.nt > 1) dma_issue(k, 1, 1);
    const int row = k.mb * BM + wave * 32 + qi;
    int qoff = row * (int)p.qs_n * 2 + hi * 16;
    int q_rows = p.Nq;                                           // (read by the packed and varlen-q forms only)
    if constexpr (VQ) {
      q_rows = vq_rows;
      if (k.mb * BM >= q_rows) {                                 // no row of the sequence in this block: nothing is requested
#pragma unroll
        for (int s = 0; s < DS; ++s) qf[s] = __builtin_bit_cast(X8, u32x4{0u, 0u, 0u, 0u});
        return;
      }
      if constexpr (!PACK) qoff = row < q_rows ? qoff : (int)TFA_OOB;
    }
    if constexpr (PACK) {
      // row = t * G + g lies at t * qs_n + g * q_hs behind the head group's base: the descriptor's extent bounds the group, not the rows — the rows behind the
      // last one (which would alias rows of the next positions' heads) are sent out of range here
      const auto& pp = KvcPackView<PACK>::of(p);
      const int t = fd_div(row, pp.pk_fd_g), g = row - t * pp.pk_g;
      qoff = row < q_rows ? (t * (int)p.qs_n + g * (int)pp.q_hs) * 2 + hi * 16 : (int)TFA_OOB;
    }
#pragma unroll
    for (int s = 0; s < DS; ++s) {
      u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(k.q_rs, (2 * s + hi) * 8 < p.dv ? qoff + s * 32 : (int)TFA_OOB, 0, 0);
      qf[s] = __builtin_bit_cast(X8, t);
    }
  };

  int item = blockIdx.x, pass = 0, nt_total = 0;
  bool first = true;
  if (item >= nitems) return;
  Blk cur;
  decode(item, pass, cur);
  if constexpr (SCHED) {
    if (sc_dead) return;                                         // behind the list's end (one item per workgroup: the whole workgroup leaves, in front of its first request)
  }
  prefetch(cur);

  while (true) {
    const int nt = cur.nt;
    nt_total += nt;
    const int wave_row0 = cur.mb * BM + wave * 32;
    const int my_row = wave_row0 + qi;
    // the query POSITIONS the causal bounds below are formed from: the row's own, the wave's first row's and its last valid row's.  Packed: t = row / G
    int my_t = my_row, my_g = 0, wave_t0 = wave_row0, wave_t1 = wave_row0 + 31;
    // the block's row count, first query row and positions: the launch's, or (varlen-q form) its sequence's — copies, decode() of the next block overwrites vq_*
    int nrows = p.Nq;
    const int cur_q0 = vq_q0, cur_nq = vq_nq;
    if constexpr (VQ) nrows = vq_rows;
    if constexpr (PACK) {
      const auto& pp = KvcPackView<PACK>::of(p);
      my_t = fd_div(my_row, pp.pk_fd_g);
      my_g = my_row - my_t * pp.pk_g;
      wave_t0 = fd_div(wave_row0, pp.pk_fd_g);
      int last_row = nrows - 1;
      if constexpr (VQ) last_row = nrows > 0 ? nrows - 1 : 0;
      wave_t1 = fd_div(wave_row0 + 31 < last_row ? wave_row0 + 31 : last_row, pp.pk_fd_g);
    }

    // tree form: the row's visibility word over its sequence's new keys — two dwords by the lane that owns the row, once per block; a row outside the
    // sequence loads nothing and sees what causal admits
    unsigned long long tree_w = ~0ull;
    if constexpr (TREE) {
      const auto& pt = KvcTreeView<TREE>::of(p);
      int tree_nq = KvcView<KVC>::of(p).nq_pos;
      long long tree_at = (long long)cur.bt_row * pt.tree_bs;
      if constexpr (VQ) { tree_nq = cur_nq; tree_at = (long long)cur_q0 * pt.tree_rs; }
      if (my_t < tree_nq) tree_w = pt.tree[tree_at + (long long)my_t * pt.tree_rs];
    }

    f32x16 oacc[WIDE ? 1 : DT];
    if constexpr (WIDE) g_zero();
    else {
#pragma unroll
      for (int d = 0; d < (WIDE ? 1 : DT); ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
    }
    float m_run = -1e30f;
    float l_run = 0.f;

    // tiles 0/1 and Q have been requested (prologue, or beside the previous block's epilogue)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (KV8) {
      if (nt > 0) stage_commit(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
#pragma unroll
    for (int s = 0; s < DS; ++s) {
      if (WIDE) asm volatile("" : "+a"(qf[s])); else asm volatile("" : "+v"(qf[s]));
    }
    asm volatile("s_barrier" ::: "memory");
    if (p.trace && first) t_pro = __builtin_amdgcn_s_memtime();

    const int shift = cur.shift;
    const int wave_last_tile = CAUSAL ? ((wave_t1 + shift) >= 0 ? (wave_t1 + shift) / BN : -1) : (nt - 1);
    // windowed form: the first tile the wave's first row sees (the tiles in front of it are left of every row's window), and the window's reach
    int wave_first_tile = 0, left = 0;
    if constexpr (WIN) {
      left = KvcWinView<WIN>::of(p).win_left;
      const int c = wave_t0 + shift - left;
      wave_first_tile = c > 0 ? c >> 6 : 0;
    }

    auto tile_body = [&](int j, int buf) {
      // tile j+2 goes into the buffer tile j-1 just vacated
      const bool more = (j + PD < nt) && !(AB & AB_NOSTAGE);
      if (more) dma_issue(cur, j + PD, (buf + PD) % NBUF);

      bool mine = j <= wave_last_tile;
      if constexpr (WIN) mine = mine && j >= wave_first_tile;
      if (mine) {
        const char* kb = kl + buf * TILE_BYTES;
        const char* vb = vl + buf * TILE_BYTES;

        f32x16 sacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[t][r] = 0.f;
        if constexpr (WIDE) {
          // k-steps in groups of four, the fragments of a group read one group ahead of the asm MFMAs that use them
          constexpr int GS = 4, NG = DS / GS;
          X8 kq[2][GS][2];
          auto rdk = [&](int gq, int buf) {
#pragma unroll
            for (int i = 0; i < GS; ++i)
#pragma unroll
              for (int t = 0; t < 2; ++t)
                kq[buf][i][t] = __builtin_bit_cast(X8, lds_read_b128(kb, k_rd_base + t * 32 * (D * 2) + (((2 * (gq * GS + i) + hi) ^ k_rd_swz) << 4)));
          };
          rdk(0, 0);
#pragma unroll
          for (int gq = 0; gq < NG; ++gq) {
            if (gq + 1 < NG) rdk(gq + 1, (gq + 1) & 1);
#pragma unroll
            for (int i = 0; i < GS; ++i)
#pragma unroll
              for (int t = 0; t < 2; ++t) {
                if (gq == 0 && i == 0) E::template mfma_bacc<true>(kq[0][0][t], qf[0], sacc[t]);      // (sacc was just zeroed by VALU moves)
                else E::template mfma_bacc<false>(kq[gq & 1][i][t], qf[gq * GS + i], sacc[t]);
              }
          }
          mfma_drain(sacc[0]);
          asm volatile("" : "+v"(sacc[1]));
        } else {
          X8 kf[DS][2];
#pragma unroll
          for (int s = 0; s < DS; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const int off = k_rd_base + t * 32 * (D * 2) + (((2 * s + hi) ^ k_rd_swz) << 4);
              if (AB & AB_NOKREAD) kf[s][t] = qf[(s + t) % DS];
              else kf[s][t] = __builtin_bit_cast(X8, lds_read_b128(kb, off));
            }
          if (VF & VF_PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int s = 0; s < DS; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              if (AB & AB_NOQK) asm volatile("" ::"v"(kf[s][t]));
              else sacc[t] = E::mfma(kf[s][t], qf[s], sacc[t]);
            }
          if (VF & VF_PRIO) __builtin_amdgcn_s_setprio(0);
        }

        auto rdv = [&](int s, int d) -> s16x8 {
          const char* a = vb + v_rd_base + (s * 2 * DT << 9) + (d << 9);
          const s16x4 lo = lds_read_tr16_b64(a), hh = lds_read_tr16_b64(a + 256);
          return __builtin_shufflevector(lo, hh, 0, 1, 2, 3, 4, 5, 6, 7);
        };
        s16x8 vq[WIDE ? 2 : 1][WIDE ? DT : 1];                // WIDE: the DT fragments of one 16-key slot, read one slot ahead
        if constexpr (WIDE) {
#pragma unroll
          for (int d = 0; d < DT; ++d) vq[0][d] = rdv(0, d);
        }
        s16x8 vfr[WIDE ? 1 : DT][WIDE ? 1 : 4];
#pragma unroll
        for (int s = 0; s < (WIDE ? 0 : 4); ++s)
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            const char* a = vb + v_rd_base + (s * 2 * DT << 9) + (d << 9);
            if (AB & AB_NOVREAD) {
              vfr[d][s] = __builtin_bit_cast(s16x8, qf[(d + s) % DS]);
            } else {
              s16x4 lo = lds_read_tr16_b64(a);
              s16x4 hh = lds_read_tr16_b64(a + 256);
              vfr[d][s] = __builtin_shufflevector(lo, hh, 0, 1, 2, 3, 4, 5, 6, 7);
            }
          }

        const int key0 = j * BN;
        bool need_mask = (key0 + BN > cur.nk);
        if (CAUSAL) need_mask = need_mask || (key0 + BN - 1 > wave_t0 + shift);
        if constexpr (WIN) need_mask = need_mask || (key0 < wave_t1 + shift - left);     // some row of the wave has its window's left edge inside the tile or behind it
        if constexpr (TREE) need_mask = need_mask || (key0 < shift + 64 && key0 + BN > shift);   // the tile holds new keys: [shift, shift + 64) in every chunk
        if (need_mask) {
          int lim = cur.nk - 1;
          if (CAUSAL) { const int c = my_t + shift; lim = c < lim ? c : lim; }
          lim -= key0 + 4 * hi;
          if constexpr (WIN) {
            const int llim = my_t + shift - left - (key0 + 4 * hi);                      // the first key of the tile this row sees
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int ko = 32 * t + (r & 3) + 8 * (r >> 2);
                if (ko > lim || ko < llim) sacc[t][r] = -INFINITY;
              }
          } else if constexpr (TREE) {
            // bit ko of vis: this row sees key key0 + 4 * hi + ko — the row's word moved from the new keys' origin to this lane's, ones in front of the
            // first new key and from the 64th on (a tile that holds no new key: all ones)
            const int off = shift - (key0 + 4 * hi);
            unsigned long long vis = ~0ull;
            if (off >= 0 && off < 64) vis = (tree_w << off) | ((1ull << off) - 1ull);
            else if (off < 0 && off > -64) vis = (tree_w >> -off) | ~(~0ull >> -off);
            const unsigned vis_lo = (unsigned)vis, vis_hi = (unsigned)(vis >> 32);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int ko = 32 * t + (r & 3) + 8 * (r >> 2);
                if (ko > lim || !((t ? vis_hi : vis_lo) & (1u << (ko & 31)))) sacc[t][r] = -INFINITY;
              }
          } else {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int ko = 32 * t + (r & 3) + 8 * (r >> 2);
                if (ko > lim) sacc[t][r] = -INFINITY;
              }
          }
        }

        float mloc = sacc[0][0];
        if (!(AB & AB_NOSM)) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, sacc[t][r]);
          mloc = pair_max(mloc);
        }
        const float m_new = (AB & AB_NOSM) ? m_run : fmaxf(m_run, mloc);
        const bool changed = (m_new != m_run);
        if (__any(changed)) {
          const float alpha = fast_exp2((m_run - m_new) * sc);
          l_run *= alpha;
          if constexpr (WIDE) g_scale(alpha);
          else {
#pragma unroll
            for (int d = 0; d < (WIDE ? 1 : DT); ++d)
#pragma unroll
              for (int r = 0; r < 16; ++r) oacc[d][r] *= alpha;
          }
        }
        m_run = m_new;
        const float msc = m_new * sc;
        X8 pk[4];
        float lsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float e;
            if (AB & AB_NOSM) e = sacc[t][r];
            else e = fast_exp2(fmaf(sacc[t][r], sc, -msc));
            if (!(AB & AB_NOSM)) lsum[r & 3] += e;
            pk[t * 2 + (r >> 3)][r & 7] = (T)e;
          }
        l_run += (lsum[0] + lsum[1]) + (lsum[2] + lsum[3]);

        if (VF & VF_PRIO) __builtin_amdgcn_s_setprio(1);
        if constexpr (WIDE) {
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s + 1 < 4) {
#pragma unroll
              for (int d = 0; d < DT; ++d) vq[(s + 1) & 1][d] = rdv(s + 1, d);
            }
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d == 0) g_mfma_d<T, true>(d, __builtin_bit_cast(X8, vq[s & 1][d]), pk[s]);
              else g_mfma_d<T, false>(d, __builtin_bit_cast(X8, vq[s & 1][d]), pk[s]);
            }
          }
        } else {
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int d = 0; d < (WIDE ? 1 : DT); ++d) {
              if (AB & AB_NOPV) asm volatile("" ::"v"(vfr[d][s]), "v"(pk[s]));
              else oacc[d] = E::mfma(__builtin_bit_cast(X8, vfr[d][s]), pk[s], oacc[d]);
            }
        }
        if (VF & VF_PRIO) __builtin_amdgcn_s_setprio(0);
      }

      // tile j+1 must have landed (this wave's pieces; the barrier covers everyone else's), and
      // every wave must be done reading tile j before tile j+3 overwrites it.  Counted wait: the
      // 2*PPW pieces of tile j+2 issued above may stay in flight.
      if (more && PD > 1) {
        if (PPW == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (PPW == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // e4m3 form: tile j+1 goes from the staging registers into the other buffer — every wave left it at the barrier behind tile j-1; the barrier below
      // puts the writes in front of tile j+1's reads
      if constexpr (KV8) { if (more) stage_commit((buf + PD) % NBUF); }
      if (AB & 256) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // AB_NOBARRIER (timing only)
      else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };

    if (NBUF == 3) {
      for (int j = 0; j < nt; j += 3) {
        tile_body(j, 0);
        if (j + 1 < nt) tile_body(j + 1, 1);
        if (j + 2 < nt) tile_body(j + 2, 2);
      }
    } else {
      for (int j = 0; j < nt; j += 2) {
        tile_body(j, 0);
        if (j + 1 < nt) tile_body(j + 1, 1);
      }
    }
    if (p.trace && first) t_loop = __builtin_amdgcn_s_memtime();
    first = false;

    // ---- next block of the stream ----------------------------------------------------------------
    const int cur_bh = cur.bh;
    const float cur_scale_lse = scale_lse, cur_vd = vd_w;   // e4m3 form: the finished block's descales — decode() of the next block overwrites sc / scale_lse / vd_w
    const long long o_part = (long long)cur.sp * p.o_part_stride, lse_part = (long long)cur.sp * p.lse_part_stride;   // 0 unless split
    constexpr bool LDS_EPI = !F32OUT && (VF & VF_LDSEPI);   // 16-bit O goes out through LDS as whole rows
    bool have_next;
    int pair_nmb = p.nmb;
    if constexpr (SCHED) pair_nmb = sc_nmb;                      // (still the finished block's: decode() of the next one comes below)
    if (PAIR && pass == 0 && (pair_nmb - 1 - cur.wi) != cur.wi) {
      pass = 1;
      have_next = true;
    } else {
      pass = 0;
      item += gridDim.x;
      have_next = item < nitems;
    }
    if (have_next && !LDS_EPI) {
      decode(item, pass, cur);
      prefetch(cur);            // LDS buffers are free: every wave passed the last tile's barrier
    }

    // ---- epilogue of the block just finished ------------------------------------------------------
    if constexpr (VQ) {
      if (wave_row0 - wave * 32 >= nrows) {                  // a block without rows: nothing to store; the next block of the stream has been requested above
        if (!have_next) break;
        continue;
      }
    }
    const int ob = cur_bh / p.H, oh = cur_bh - ob * p.H;
    // varlen-q form: the extent of the sequence's rows of O behind (h, q0_b) — the descriptors below end at its last row
    unsigned o_ext = (unsigned)p.o_bytes;
    if constexpr (VQ) {
      long long e = (long long)(cur_nq - 1) * p.os_n + p.dv;
      if constexpr (PACK) e += (long long)(KvcPackView<PACK>::of(p).pk_g - 1) * KvcPackView<PACK>::of(p).o_hs;
      o_ext = cur_nq > 0 ? (unsigned)(e * (F32OUT ? 4 : 2)) : 0u;
    }
    float og[WIDE ? DT : 1][16];                           // WIDE: O read out of the hand-owned AccVGPRs
    if constexpr (WIDE) {
#pragma unroll
      for (int d = 0; d < DT; ++d) g_read_d(d, og[d]);
    }
    auto ov = [&](int d, int i) -> float { return WIDE ? og[WIDE ? d : 0][i] : oacc[WIDE ? 0 : d][i]; };
    const float l_tot = pair_sum(l_run);
    const bool empty = !(l_tot > 0.f);
    const float inv = KV8 ? (empty ? 1.f : 1.f / l_tot) * cur_vd : (empty ? 1.f : 1.f / l_tot);   // e4m3 form: v_descale in fp32, in front of the one rounding of O
    if (p.lse != nullptr && hi == 0 && my_row < nrows) {
      const float lse = empty ? INFINITY : (m_run * (KV8 ? cur_scale_lse : p.scale) + __builtin_amdgcn_logf(l_tot) * 0.6931471805599453f);
      // (packed: cur_bh = b * Hk + hk and p.Nq = Nq * G, so the first two terms are the caller's (b * H + hk * G) * Nq; head g, position t follow)
      // (varlen-q: (H, total_q) — head oh, or hk * G + g packed, at row q0_b + t)
      if constexpr (VQ) {
        int lh = oh;
        if constexpr (PACK) lh = oh * KvcPackView<PACK>::of(p).pk_g + my_g;
        p.lse[lse_part + (long long)lh * KvcVqView<VQ>::of(p).vq_total_q + cur_q0 + my_t] = lse;
      }
      else if constexpr (PACK) p.lse[lse_part + (long long)cur_bh * p.Nq + my_g * KvcPackView<PACK>::of(p).nq_pos + my_t] = lse;
      else p.lse[lse_part + (long long)cur_bh * p.Nq + my_row] = lse;
    }
    if (F32OUT) {
      float* obase = reinterpret_cast<float*>(p.o) + o_part + ob * p.os_b + oh * p.os_h;
      if constexpr (VQ) obase += (long long)cur_q0 * p.os_n;
      auto o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)obase, 0, o_ext, 0x00020000);
      int ooff = my_row * (int)p.os_n * 4 + hi * 16;
      if constexpr (VQ && !PACK) ooff = my_row < nrows ? ooff : (int)TFA_OOB;
      if constexpr (PACK) ooff = my_row < nrows ? (my_t * (int)p.os_n + my_g * (int)KvcPackView<PACK>::of(p).o_hs) * 4 + hi * 16 : (int)TFA_OOB;   // the caller's (b, h, t) row
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 v4 = {ov(d, 4 * g + 0) * inv, ov(d, 4 * g + 1) * inv, ov(d, 4 * g + 2) * inv, ov(d, 4 * g + 3) * inv};
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v4), o_rs, d * 32 + g * 8 + hi * 4 < p.dv ? ooff + (d * 32 + g * 8) * 4 : (int)TFA_OOB, 0, 0);
        }
    } else if (LDS_EPI) {
      // Each lane holds 4-element pieces of ONE row scattered over 16 registers groups: stored directly that is
      // 16 eight-byte stores per lane to 32 different rows per instruction.  Instead the wave transposes its
      // 32 x D tile through its own slice of the (now idle) K buffers — 16-byte chunk index XOR row, as for K —
      // and writes whole rows: 1 KiB contiguous per store instruction.
      T* obase = reinterpret_cast<T*>(p.o) + o_part + ob * p.os_b + oh * p.os_h;
      auto o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)obase, 0, (unsigned)p.o_bytes, 0x00020000);
      typedef __attribute__((ext_vector_type(4))) T t4;
      char* const ow = smem + wave * (32 * D * 2);
      constexpr int CH = D / 8;                      // 16-byte chunks per row
      const int osw = (CH == 16) ? (qi & 15) : (qi & 7);
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          t4 v4 = {(T)(ov(d, 4 * g + 0) * inv), (T)(ov(d, 4 * g + 1) * inv), (T)(ov(d, 4 * g + 2) * inv), (T)(ov(d, 4 * g + 3) * inv)};
          const int c = d * 4 + g;
          *reinterpret_cast<u32x2*>(ow + qi * (D * 2) + ((c ^ osw) << 4) + hi * 8) = __builtin_bit_cast(u32x2, v4);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private slice: no barrier needed
      constexpr int RPI = 64 / CH;                   // rows per store instruction (4 at D=128, 8 at D=64)
#pragma unroll
      for (int i = 0; i < 32 / RPI; ++i) {
        const int r = i * RPI + lane / CH, cpos = lane % CH;
        const int c = cpos ^ ((CH == 16) ? (r & 15) : (r & 7));
        u32x4 v = *reinterpret_cast<const u32x4*>(ow + r * (D * 2) + (cpos << 4));
        __builtin_amdgcn_raw_buffer_store_b128(v, o_rs, c * 8 < p.dv ? (wave_row0 + r) * (int)p.os_n * 2 + (c << 4) : (int)TFA_OOB, 0, 0);
      }
      if (have_next) {
        // the next block's DMA will overwrite these slices: every wave must have read its rows back
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        decode(item, pass, cur);
        prefetch(cur);
      }
    } else {
      T* obase = reinterpret_cast<T*>(p.o) + o_part + ob * p.os_b + oh * p.os_h;
      if constexpr (VQ) obase += (long long)cur_q0 * p.os_n;
      auto o_rs = __builtin_amdgcn_make_buffer_rsrc((void*)obase, 0, o_ext, 0x00020000);
      int ooff = my_row * (int)p.os_n * 2 + hi * 8;
      if constexpr (VQ && !PACK) ooff = my_row < nrows ? ooff : (int)TFA_OOB;
      if constexpr (PACK) ooff = my_row < nrows ? (my_t * (int)p.os_n + my_g * (int)KvcPackView<PACK>::of(p).o_hs) * 2 + hi * 8 : (int)TFA_OOB;
      typedef __attribute__((ext_vector_type(4))) T t4;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          t4 v4 = {(T)(ov(d, 4 * g + 0) * inv), (T)(ov(d, 4 * g + 1) * inv), (T)(ov(d, 4 * g + 2) * inv), (T)(ov(d, 4 * g + 3) * inv)};
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v4), o_rs, d * 32 + g * 8 + hi * 4 < p.dv ? ooff + (d * 32 + g * 8) * 2 : (int)TFA_OOB, 0, 0);
        }
    }
    if (!have_next) break;
  }

  if (p.trace) {
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    if (tid == 0) {
      unsigned long long* t = p.trace + (size_t)blockIdx.x * 8;
      t[0] = t_start; t[1] = t_pro; t[2] = t_loop; t[3] = t_end;
      t[4] = (unsigned long long)nt_total;
      t[5] = (unsigned long long)__builtin_amdgcn_s_getreg(63508) | ((unsigned long long)__builtin_amdgcn_s_getreg(63492) << 32);   // XCC_ID | HW_ID << 32
      t[6] = __builtin_amdgcn_s_memrealtime() - rt_start;   // 100 MHz ticks over the same span as t[3] - t[0] shader cycles
      t[7] = (unsigned long long)blockIdx.x;
    }
  }
