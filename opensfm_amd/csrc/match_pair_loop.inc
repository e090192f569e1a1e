// match_pair_loop.inc -- the body of a fused matcher kernel: what every workgroup of the resident grid does.  Included inside the
// kernel's braces by match.hip (match_fused_kernel<FQ>, SHAPE 32) and match16.hip (match_sweep16_kernel, SHAPE 16), with MatchArgs a,
// bool FQ and int SHAPE in scope: the kernels differ in the sweep's MFMA shape only, and a body shared as a function did not leave
// the 32x32x32 kernel's code as it was (tests/test_kernel_budgets*.py pin it).
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  QueryPassShared sh;
  sh.bbuf = smem;                               // [2][32 KiB]
  sh.hbuf = (int *)(smem + 2 * kChunkBytes4);  // [2][256]
  int *misc = (int *)(smem + 2 * kChunkBytes4) + 2 * kChunkCols4;  // [16]
  int *hdr = misc + 16;                                            // [16] header of the next pair (9 used)
  unsigned short *resA = (unsigned short *)(hdr + 16);             // [ncap] per feature of image A
  unsigned short *resB = resA + a.ncap;                            // [ncap] per feature of image B
  unsigned short *cand = resB + a.ncap;                            // [ncap] candidate list (features of B)

  const int xcd = blockIdx.x & 7;  // the eighth of the pair list this block starts in
  const int8_t *tiles_pad = a.tiles + a.pad_tile * OSFM_TILE_BYTES;  // the store's first slack tile: zero descriptors, padding norms
  const int32_t *hneg_pad = a.hneg + a.pad_tile * 32;
  OSFM_TICK(tw0)
#ifdef OSFM_DBG_PHASES
  unsigned long long t_prev = tw0;  // end of the previous pair's last write (first pair: the workgroup's first instruction)
#endif
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x == 0) {
    hdr[8] = 0;
    fetch_pair_header(a, xcd, hdr);
  }
  __syncthreads();
  for (;;) {
  const int tid = fresh_tid(wave);  // (for the top of the pair only: every later phase makes its own)
  const long p = __builtin_amdgcn_readfirstlane(hdr[0]);
  if (p < 0) break;  // the list is used up
  if (__builtin_amdgcn_readfirstlane(hdr[7]) == 0) {  // the previous pass A had one chunk only: the counts and offsets are still to be fetched
    __syncthreads();
    if (tid == 0) finish_pair_header(a, hdr);
    __syncthreads();
  }
  const int img1 = __builtin_amdgcn_readfirstlane(hdr[1]), img2 = __builtin_amdgcn_readfirstlane(hdr[2]);
  const int n1 = __builtin_amdgcn_readfirstlane(hdr[3]), n2 = __builtin_amdgcn_readfirstlane(hdr[4]);
  const long off1 = __builtin_amdgcn_readfirstlane(hdr[5]), off2 = __builtin_amdgcn_readfirstlane(hdr[6]);
  if (tid == 0) {
    misc[8] = 0;
    misc[9] = 0;   // hit word of pass A
    misc[10] = 0;  // hit word of pass B
  }
  __syncthreads();  // the header is read (thread 0 may overwrite it), the previous pair's results are no longer looked at
  if (n1 < 2 || n2 < 2) {  // matching.py:363-374 / knnMatch returns < 2 neighbours
    if (tid == 0) {
      a.out_counts[p] = 0;
      a.out_flags[p] = 0;
      fetch_pair_header(a, xcd, hdr);
    }
    __syncthreads();
#ifdef OSFM_DBG_PHASES
    {  // a bucket of its own, so that the next pair's boundary does not take this pair's handling (a header fetched in one go) with it
      OSFM_TICK(te)
      OSFM_PHASE(19, t_prev, te)
      if (threadIdx.x == 0) atomicAdd(&g_phase[20], 1ull);
      t_prev = te;
    }
#endif
    continue;
  }
  // symmetric: A = second image (rows of the big pass), B = first image (streamed, shared in L2)
  const bool rows_second = a.symmetric || a.query_second;
  const int imgA = rows_second ? img2 : img1, imgB = rows_second ? img1 : img2;
  const int nA = rows_second ? n2 : n1, nB = rows_second ? n1 : n2;
  const long offA = rows_second ? off2 : off1, offB = rows_second ? off1 : off2;
  const int8_t *tilesA = a.tiles + offA * OSFM_TILE_BYTES;
  const int8_t *tilesB = a.tiles + offB * OSFM_TILE_BYTES;
  const int32_t *normA = a.norms + offA * 32;
  const int32_t *normB = a.norms + offB * 32;
  const int32_t *hnegA = a.hneg + offA * 32;
  const int32_t *hnegB = a.hneg + offB * 32;
  // (no clear of resA: pass A writes every slot of image A, kNone included; resB is cleared where the candidate list needs it)
  // FQ: the float rows of the two images and the quantisation error bound of the pair
  OSFM_TICK(tq0)
  const float *descA = FQ ? a.descf + offA * (long)(32 * OSFM_DESC_DIM) : nullptr;
  const float *descB = FQ ? a.descf + offB * (long)(32 * OSFM_DESC_DIM) : nullptr;
  const double eps = FQ ? (double)a.qerr[imgA] + (double)a.qerr[imgB] : 0.0;
  // any: some query of the last pass run got a partner.  Without one the pair is empty (98 % of an exhaustive list): candidate
  // list, pass B and the emission scan are skipped; the count and the flag (which may still ask for the exact re-run) are written
  int any = 0;
  // integer store: flag = the pair has to be re-run by the exact kernel; float store: the number of queries evaluated in float
  auto flush_flag = [&](int f) {
    if (FQ) {
      if ((fresh_tid(wave) & 63) == 0 && f) atomicAdd(&misc[8], f);
    } else if (f) {
      misc[8] = 1;
    }
  };
  int flag = query_pass<false, FQ, SHAPE>(sh, tilesA, normA, nA, nA, nullptr, tilesB, normB, hnegB, nB, tiles_pad, hneg_pad, resA, a.ratio, fresh_tid(wave),
                                   descA, descB, eps, misc + 9, any, NextPairFetch{a, xcd, hdr, fresh_tid(wave), 0});
  OSFM_TICK(tq1)
  OSFM_PHASE(10, tq0, tq1)  // pass A
  if (a.symmetric && any) {
    // candidates: the features of B that some row of A chose.  resB doubles as the mark array
    // (0 = chosen) until the candidate list is built, in ascending feature order.
    const int tid = fresh_tid(wave), lane = tid & 63, w = tid >> 6;
    for (int j = tid; j < nB; j += kThreads) resB[j] = kNone;  // (only here: nothing reads resB in a pair without candidates)
    __syncthreads();
    for (int q = tid; q < nA; q += kThreads) {
      const int b = resA[q];
      if (b != kNone) resB[b] = 0;
    }
    __syncthreads();
    int base = 0;
    for (int j0 = 0; j0 < nB; j0 += kThreads) {
      const int j = j0 + tid;
      const bool m = j < nB && resB[j] == 0;
      const unsigned long long bal = __ballot(m);
      if (lane == 0) misc[w] = __popcll(bal);
      __syncthreads();
      int woff = 0, total = 0;
#pragma unroll
      for (int w2 = 0; w2 < kWaves; ++w2) {
        const int cnt = misc[w2];
        woff += (w2 < w) ? cnt : 0;
        total += cnt;
      }
      if (m) {
        cand[base + woff + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)j;
        resB[j] = kNone;
      }
      base += total;
      __syncthreads();
    }
    const int nK = base;
    OSFM_TICK(tq2)
    OSFM_PHASE(11, tq1, tq2)  // candidate list
    // (nK > 0: some resA named a feature of B)
    flush_flag(flag);  // (not carried through pass B in a vector register)
    flag = query_pass<true, FQ, SHAPE>(sh, tilesB, normB, nB, nK, cand, tilesA, normA, hnegA, nA, tiles_pad, hneg_pad, resB, a.ratio, fresh_tid(wave), descB, descA,
                                 eps, misc + 10, any, NoFetch{});
  }
  OSFM_TICK(tq3)
  OSFM_PHASE(12, tq1, tq3)  // candidate list + pass B
  flush_flag(flag);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the next pair's header has landed in LDS (wave 0's DMAs)
  __syncthreads();
  if (fresh_tid(wave) == 0) a.out_flags[p] = misc[8];
  // ---- ordered emission: over the features of the pair's first image, or (query_second) of its second image,
  //      the order in which the reference lists the matches of match_flann (matching.py:697) ----
  if (!any) {
    if (fresh_tid(wave) == 0) a.out_counts[p] = 0;
  } else {
    const int tid = fresh_tid(wave), lane = tid & 63, w = tid >> 6;
    const bool qs = !a.symmetric && a.query_second;
    const unsigned short *res1 = a.symmetric ? resB : resA;  // indexed by the emission feature -> its partner
    const unsigned short *res2 = a.symmetric ? resA : nullptr;
    const int nE = qs ? n2 : n1;
    int base = 0;
    for (int j0 = 0; j0 < nE; j0 += kThreads) {
      const int j = j0 + tid;
      bool m = false;
      int r = kNone;
      if (j < nE) {
        r = res1[j];
        m = (r != kNone) && (!res2 || res2[r] == j);
      }
      const unsigned long long bal = __ballot(m);
      const int prefix = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) misc[w] = __popcll(bal);
      __syncthreads();
      int woff = 0, total = 0;
#pragma unroll
      for (int w2 = 0; w2 < kWaves; ++w2) {
        const int cnt = misc[w2];
        woff += (w2 < w) ? cnt : 0;
        total += cnt;
      }
      if (m) {
        const int k = base + woff + prefix;
        // low half = feature of image 1, high half = feature of image 2
        if (k < a.cap) a.out_matches[p * a.cap + k] = qs ? ((uint32_t)r | ((uint32_t)j << 16)) : ((uint32_t)j | ((uint32_t)r << 16));
      }
      base += total;
      __syncthreads();
    }
    if (tid == 0) a.out_counts[p] = base;
  }
  OSFM_TICK(tq4)
  OSFM_PHASE(13, tq3, tq4)  // emission
  OSFM_PHASE(14, tq0, tq4)
#ifdef OSFM_DBG_PHASES
  if (threadIdx.x == 0) atomicAdd(&g_phase[15], 1ull);
  OSFM_PHASE(16, t_prev, tq0)  // boundary: from the previous pair's last write to this pair's pass A (ticket, header, pointers)
  t_prev = tq4;
#endif
  }  // pairs
#ifdef OSFM_DBG_PHASES
  if (threadIdx.x == 0) {
    atomicAdd(&g_phase[17], wall_clock64() - tw0);  // the workgroup's whole life
    atomicAdd(&g_phase[18], 1ull);
  }
#endif
