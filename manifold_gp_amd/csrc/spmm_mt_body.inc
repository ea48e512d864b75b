// Body of spmm_mt_kernel / spmm_mt_cbv_kernel (csrc/spmm.hip), included inside the two kernels with PRE (template
// parameter) and CBV (constexpr: SpmmArgs::cbv is read) in scope.  Kept as text rather than as an inline function:
// a function taking the kernel's arguments by reference makes the compiler copy them to LDS.
  constexpr int LR = PRE ? 12 : 8;      // loads per block request
  if (p.skip && *p.skip) return;
  if (p.tick && blockIdx.x == 0 && threadIdx.x == 0) *p.tick += 1;
  const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
  const int lb = mgp_xcd_block(blockIdx.x, gridDim.x);
  const int w = __builtin_amdgcn_readfirstlane(lb * (kBlock / 64) + (int)(threadIdx.x >> 6));
  const int t = w / m.NCB, cb = w % m.NCB;           // the column blocks of a tile side by side: they share its image
  const int C = p.C;
  if (t >= m.T && !p.dot_partials) return;           // (with dot partials every wave of the workgroup meets at the barrier below)
  mgp_v4f ds = {0.f, 0.f, 0.f, 0.f};                 // this lane's share of sum_rows dotw * y for columns c0 .. c0 + 3
  MT_STAMP(0);
  if (t < m.T) {
  const int blk0 = __builtin_amdgcn_readfirstlane(m.sptr[t]) >> 2, blk1 = __builtin_amdgcn_readfirstlane(m.sptr[t + 1]) >> 2;
  const int64_t nx = p.n + p.goff;                   // rows of X the columns can name (host side: goff == 0)
#if defined(MGP_MT_LAB) && (MGP_MT_LAB & 2)     // lab (tools/lab/mt_bounds.sh): every X request out of range -> zeros, no memory traffic
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), (short)0, 0, 0x00020000);
#else
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), (short)0, (int)(nx * C * 4), 0x00020000);
#endif
  const __amdgpu_buffer_rsrc_t rimg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(m.img), (short)0, m.img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rdic = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(m.dcol), (short)0, m.dic_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rpre = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(PRE ? p.pre : p.X), (short)0, (int)(nx * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rdiag = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.diag), (short)0, (int)(p.n * 4), 0x00020000);
#if defined(MGP_MT_LAB) && (MGP_MT_LAB & 4)     // lab: every X request goes to row 0 (always cached)
  const int lane4 = lane * 4, rowbytes = 0, joff = cb * 256 + j * 16;
#else
  const int lane4 = lane * 4, rowbytes = C * 4, joff = cb * 256 + j * 16;
#endif
  const int c0 = 64 * cb + 4 * j;                    // acc[e][r]: row 16 t + 4 kq + r, column c0 + e
  mgp_v4f acc[4], ex[4];
  float ed[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { acc[e] = mgp_v4f{0.f, 0.f, 0.f, 0.f}; ex[e] = mgp_v4f{0.f, 0.f, 0.f, 0.f}; ed[e] = 0.f; }
  MtBuf<PRE> buf0, buf1, buf2, buf3;
  int dq0, dq1, dq2;          // column-list batches of the body in hand, of the next one, and the one in flight
  const int dic0 = blk0 * 64, img0 = blk0 * 1024;      // byte offsets of the tile's first block
  asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(dq0) : "v"(lane4), "s"(rdic), "s"(dic0));
  asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:256" : "=v"(dq1) : "v"(lane4), "s"(rdic), "s"(dic0));
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(dq0), "+v"(dq1));
  mt_request<PRE>(buf0, dq0, 0, kq, joff, rowbytes, img0, rimg, rx, rpre, lane4);
  mt_request<PRE>(buf1, dq0, 4, kq, joff, rowbytes, img0 + 1024, rimg, rx, rpre, lane4);
  mt_request<PRE>(buf2, dq0, 8, kq, joff, rowbytes, img0 + 2048, rimg, rx, rpre, lane4);
  {
    // the epilogue's operands: the X block of the tile's own rows (16 bytes per lane and row) and the diagonal
    int offx[4], offd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * kq + r;
      // (rows past n / columns past C: in range of the descriptor or answered with 0; 24-bit multiply as in mt_request)
      offx[r] = (int)__umul24((unsigned)row, (unsigned)(C * 4)) + c0 * 4;
      offd[r] = row * 4;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(ex[r]) : "v"(offx[r]), "s"(rx));
      asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "+v"(ed[r]) : "v"(offd[r]), "s"(rdiag));
    }
    asm volatile("" :: "v"(offx[0]), "v"(offx[1]), "v"(offx[2]), "v"(offx[3]), "v"(offd[0]), "v"(offd[1]), "v"(offd[2]), "v"(offd[3]));
  }
  MT_STAMP(1);
  for (int k = blk0; k < blk1 - 4; k += 4) {
    const int so = k * 1024, sd = k * 64;
    asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:512" : "=v"(dq2) : "v"(lane4), "s"(rdic), "s"(sd));
    mt_wait<2 * LR + 1, PRE>(buf0);
    mt_request<PRE>(buf3, dq0, 12, kq, joff, rowbytes, so + 3 * 1024, rimg, rx, rpre, lane4);
    __builtin_amdgcn_sched_barrier(0);      // requests stay in front of the block's MFMAs (left alone, the scheduler sinks them)
    mt_mfma<PRE>(buf0, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<2 * LR + 1, PRE>(buf1);
    mt_request<PRE>(buf0, dq1, 0, kq, joff, rowbytes, so + 4 * 1024, rimg, rx, rpre, lane4);
    __builtin_amdgcn_sched_barrier(0);
    mt_mfma<PRE>(buf1, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<2 * LR + 1, PRE>(buf2);
    mt_request<PRE>(buf1, dq1, 4, kq, joff, rowbytes, so + 5 * 1024, rimg, rx, rpre, lane4);
    __builtin_amdgcn_sched_barrier(0);
    mt_mfma<PRE>(buf2, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<2 * LR, PRE>(buf3);
    mt_request<PRE>(buf2, dq1, 8, kq, joff, rowbytes, so + 6 * 1024, rimg, rx, rpre, lane4);
    __builtin_amdgcn_sched_barrier(0);
    mt_mfma<PRE>(buf3, acc);
    __builtin_amdgcn_sched_barrier(0);
    dq0 = dq1;
    // the batch requested at the top of this body is older than R(k+3), which wait(k+3) has seen land: 3 LR = R(k+4..k+6)
    // waits for nothing new, it only tells the compiler where dq2 becomes readable
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(dq2) : "n"(3 * LR));
    dq1 = dq2;
  }
  // ---- the tile's LAST body, peeled: in flight at the top R(k) R(k+1) R(k+2); behind the one request left, R(k+1) R(k+2) R(k+3)
  {
    const int so = (blk1 - 4) * 1024;
    mt_wait<2 * LR, PRE>(buf0);
    mt_request<PRE>(buf3, dq0, 12, kq, joff, rowbytes, so + 3 * 1024, rimg, rx, rpre, lane4);
    __builtin_amdgcn_sched_barrier(0);
    mt_mfma<PRE>(buf0, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<2 * LR, PRE>(buf1);
    mt_mfma<PRE>(buf1, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<LR, PRE>(buf2);
    mt_mfma<PRE>(buf2, acc);
    __builtin_amdgcn_sched_barrier(0);
    mt_wait<0, PRE>(buf3);
    mt_mfma<PRE>(buf3, acc);
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(dq0), "+v"(dq1));
  mt_wait<0, PRE>(buf0); mt_wait<0, PRE>(buf1); mt_wait<0, PRE>(buf2);
#pragma unroll
  for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(ex[r]), "+v"(ed[r]));
  MT_STAMP(2);
#ifdef MGP_MT_STAMP
  if (m.stamps && lane == 0) {
    m.stamps[(size_t)w * 8 + 4] = (unsigned long long)(blk1 - blk0);
    m.stamps[(size_t)w * 8 + 5] = (unsigned long long)__builtin_amdgcn_s_getreg(63492);     // HW_REG_HW_ID
    m.stamps[(size_t)w * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg(63508);     // HW_REG_XCC_ID
  }
#endif
  if (c0 < C) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = (int64_t)16 * t + 4 * kq + r;
      if (row < p.n) {
        const int64_t gr = row + p.goff;
        mgp_v4f xs = ex[r];
        if (PRE) xs *= p.pre[gr];
        const mgp_v4f av = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
        const mgp_v4f lx = ed[r] * xs - av;
        mgp_v4f tt = p.a * xs + p.b * lx;
        if (p.post) tt *= p.post[gr];
        mgp_v4f y = p.co * tt;
        if (p.base) y += (CBV ? p.cbv[gr] : p.cb) * *reinterpret_cast<const mgp_v4f*>(p.base + gr * C + c0);
        *reinterpret_cast<mgp_v4f*>(p.Y + gr * C + c0) = y;
        if (p.dot_partials) {
          const mgp_v4f dw = (p.dotw == p.X) ? ex[r] : *reinterpret_cast<const mgp_v4f*>(p.dotw + gr * C + c0);
          ds += dw * y;
        }
      }
    }
  }
#ifdef MGP_MT_STAMP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  MT_STAMP(3);
  }   // t < m.T
  if (p.dot_partials) {
    // per workgroup and column: lanes kq = 1..3 onto kq = 0 (fixed order), then the workgroup's waves of the column's block in
    // wave order.  Any four consecutive waves hold every column block (NCB <= 4), except past the last tile: zeros there.
    __shared__ float red[kBlock / 64][64];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = ds[e];
      v += __shfl_down(v, 16, 64);
      v += __shfl_down(v, 32, 64);
      if (kq == 0) red[wave][4 * j + e] = v;
    }
    __syncthreads();
    const int w0 = lb * (kBlock / 64);
    for (int c = threadIdx.x; c < C; c += kBlock) {
      float tsum = 0.f;
#pragma unroll
      for (int wv = 0; wv < kBlock / 64; ++wv)
        if ((w0 + wv) % m.NCB == c / 64 && (w0 + wv) / m.NCB < m.T) tsum += red[wv][c & 63];
      p.dot_partials[(int64_t)lb * C + c] = tsum;
    }
  }
