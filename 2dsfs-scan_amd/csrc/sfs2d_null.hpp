// sfs2d_null.hpp -- the bootstrap null of T2D / T1D (included by sfs2d_kernels.hpp, inside sfs2dk).
//
// A replicate window of a task (pool, m) is m SNPs drawn with replacement from the pool's SNP range
// and evaluated as eval_exact evaluates a real window against the pool's background table (DESIGN.md
// section 14).  Draw j of replicate r:
//   c = philox4x32((j >> 1, r, m, pool + 1), (seed lo, seed hi));  x64 = c.x | c.y << 32 (j even),
//   c.z | c.w << 32 (j odd);  SNP index = lo + mulhi64(x64, n)
// -- integers only, a function of (seed, pool, m, r, j) and of nothing else (sfs2d.null.draw_indices is
// the host twin).  The drawn windows exist only in registers: one Philox call gives a lane two draws,
// the first NULL_KEEP calls' SNP words stay in registers for the take-and-clear pass (m <= 128 NULL_KEEP:
// one gather per draw), later ones are drawn again.
//
//   k_null      one wavefront per (task, replicate); a workgroup is as many wavefronts as the host fits
//               histograms into 64 KB of LDS (8 for small grids, 1 for 201 x 151); grid-stride over the
//               records, so a wave zeroes its histograms once (the take pass leaves them zero)
//   k_null_blk  the same for a block null (sfs2d_plan_null_run_blocks, block length b >= 2): draw i above is
//               the START s_i of block i, and draw j = i b + k (k < b) is SNP lo + (s_i + k) mod n -- runs of
//               consecutive SNPs of a circular pool, the last one cut at m.  Lane l owns draws l + 64 t; lane q
//               makes Philox call q once per round of 128 blocks (= 2 b rows of 64 draws, so rounds begin on
//               row boundaries) and a draw fetches its block's start by a lane shuffle; (j / b, j mod b) is
//               carried from row to row.  Histograms, evaluation and records as k_null
//   k_null_tail the last step of a sliced plan's table (k_bg_slice ran without its tail and k_scan_w's
//               prologue keeps the result in LDS): numpy's tree over the leaf sums, scipy's p[-1] rule on
//               the last inner 2D bin and the head, for every chromosome, as k_bg_slice's tail does
#pragma once

struct NullTask {   // one (pool, m): SNPs [lo, lo + n) of the data set, m draws per replicate
  uint32_t lo, n, m;
  int32_t pool;     // chromosome index, -1 = the whole data set
};
static_assert(sizeof(NullTask) == 16, "null tasks are 16 bytes");

constexpr int NULL_KEEP = 4;      // Philox calls per lane whose two SNP words stay in registers
constexpr int NULL_MAX_WAVES = 8;

__device__ __forceinline__ uint32_t null_index(uint32_t xlo, uint32_t xhi, uint32_t lo, uint32_t n) {
  const unsigned long long x = (unsigned long long)xlo | ((unsigned long long)xhi << 32);
  return lo + (uint32_t)__umul64hi(x, (unsigned long long)n);   // n < 2^32: the high word is < n
}

// words per wavefront of k_null's LDS: 2D bins (u16 pairs when P16) | folded pop-1 1D | pop-2 1D, 16-B rows
__host__ __device__ __forceinline__ int null_wave_words(int nb2, int n1p, int n2p, bool p16) {
  return ((p16 ? (nb2 + 1) / 2 : nb2) + (n1p + 1) + (n2p + 1) + 3) & ~3;
}

template <bool P16, bool CNT>
__global__ __launch_bounds__(NULL_MAX_WAVES* WAVE) void k_null(KParams P, const uint32_t* __restrict__ src,
                                                               const NullTask* __restrict__ tasks, uint32_t R,
                                                               unsigned long long nrec, uint2 key,
                                                               const PL* __restrict__ tab,
                                                               const BgHead* __restrict__ head, int bg_per_chrom,
                                                               const double* __restrict__ lnx,
                                                               sfs2d_window* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const int h2w = P16 ? (P.nb2 + 1) / 2 : P.nb2;
  const int per = null_wave_words(P.nb2, P.n1p, P.n2p, P16);
  uint32_t* H2 = lds + (size_t)wv * per;
  uint32_t* H1a = H2 + h2w;
  uint32_t* H1b = H1a + (P.n1p + 1);
  for (int k = lane; k < per; k += WAVE) H2[k] = 0u;
  group_sync<WAVE>();
  for (unsigned long long g = (unsigned long long)blockIdx.x * nwv + wv; g < nrec; g += (unsigned long long)gridDim.x * nwv) {
    const uint32_t t = (uint32_t)(g / R), r = (uint32_t)(g - (unsigned long long)t * R);
    const NullTask tk = tasks[t];
    const int bg = bg_per_chrom ? tk.pool : 0;
    const TabGlobal T{tab + (size_t)bg * P.nt};
    const BgHead hb = head[bg];
    const bool floatv = hb.flags & BGF_FLOATV;
    const uint32_t npair = (tk.m + 1u) >> 1;
    // the SNP words of draws 2q and 2q + 1 (0 -- a word that counts nowhere -- for a draw past m)
    auto words = [&](uint32_t q, uint32_t& w0, uint32_t& w1) {
      const uint4 c = philox4x32(make_uint4(q, r, tk.m, (uint32_t)(tk.pool + 1)), key);
      w0 = snp_word<CNT>(P, src, null_index(c.x, c.y, tk.lo, tk.n));
      w1 = 2u * q + 1u < tk.m ? snp_word<CNT>(P, src, null_index(c.z, c.w, tk.lo, tk.n)) : 0u;
    };
    uint32_t c_var = 0, c2 = 0, c_last = 0, c1a = 0, c1b = 0;
    auto add = [&](uint32_t w) {
      const uint32_t k2 = bin_k2(w), g1 = bin_g1(w), g2 = bin_g2(w);
      c_var += (w & B_VAR) ? 1u : 0u;
      c_last += (w & B_LAST) ? 1u : 0u;
      if (k2) { ++c2; h2_add<P16>(H2, k2); }
      if (g1) { ++c1a; atomicAdd(&H1a[g1], 1u); }
      if (g2) { ++c1b; atomicAdd(&H1b[g2], 1u); }
    };
    uint32_t kw[2 * NULL_KEEP];
#pragma unroll
    for (int i = 0; i < NULL_KEEP; ++i) {
      const uint32_t q = (uint32_t)lane + (uint32_t)(WAVE * i);
      kw[2 * i] = 0u;
      kw[2 * i + 1] = 0u;
      if (q < npair) words(q, kw[2 * i], kw[2 * i + 1]);
      add(kw[2 * i]);
      add(kw[2 * i + 1]);
    }
    for (uint32_t q = (uint32_t)lane + (uint32_t)(WAVE * NULL_KEEP); q < npair; q += WAVE) {
      uint32_t w0, w1;
      words(q, w0, w1);
      add(w0);
      add(w1);
    }
    group_sync<WAVE>();
    const unsigned long long r0 = wave_sum_u64((unsigned long long)c2 | ((unsigned long long)c_last << 32));
    const unsigned long long r1 = wave_sum_u64((unsigned long long)c1a | ((unsigned long long)c1b << 32));
    WinOut o;
    o.n2 = (uint32_t)r0;
    o.n2_all = o.n2 + (uint32_t)(r0 >> 32);
    o.n1a = (uint32_t)r1;
    o.n1b = (uint32_t)(r1 >> 32);
    o.snp_count = wave_sum_u(c_var);
    const double N2 = (double)o.n2, N1a = (double)o.n1a, N1b = (double)o.n1b;
    double s2 = 0.0, sa = 0.0, sb = 0.0;
    bool q2 = true, qa = true, qb = true;   // x_k/N == p_k bitwise on every touched bin (eval_exact)
    auto take = [&](uint32_t w) {
      const uint32_t k2 = bin_k2(w), g1 = bin_g1(w), g2 = bin_g2(w);
      if (k2) {
        const uint32_t x = h2_take<P16>(H2, k2);
        if (x) {
          const PL e = T.at(k2);
          s2 += (double)x * (lnx_of(lnx, x) - e.lp);
          q2 &= prop_ok(x, N2, e.v, hb.B2, floatv);
        }
      }
      if (g1) {
        const uint32_t x = atomicExch(&H1a[g1], 0u);
        if (x) {
          const PL e = T.at(P.t1a + g1);
          sa += (double)x * (lnx_of(lnx, x) - e.lp);
          qa &= prop_ok(x, N1a, e.v, hb.B1a, floatv);
        }
      }
      if (g2) {
        const uint32_t x = atomicExch(&H1b[g2], 0u);
        if (x) {
          const PL e = T.at(P.t1b + g2);
          sb += (double)x * (lnx_of(lnx, x) - e.lp);
          qb &= prop_ok(x, N1b, e.v, hb.B1b, floatv);
        }
      }
    };
#pragma unroll
    for (int i = 0; i < NULL_KEEP; ++i) {
      take(kw[2 * i]);
      take(kw[2 * i + 1]);
    }
    for (uint32_t q = (uint32_t)lane + (uint32_t)(WAVE * NULL_KEEP); q < npair; q += WAVE) {
      uint32_t w0, w1;
      words(q, w0, w1);   // the same draws again: nothing of a replicate window is staged in memory
      take(w0);
      take(w1);
    }
    s2 = wave_sum_d(s2);
    sa = wave_sum_d(sa);
    sb = wave_sum_d(sb);
    const unsigned long long bad = wave_sum_u64((unsigned long long)(!q2) | ((unsigned long long)(!qa) << 21) |
                                                ((unsigned long long)(!qb) << 42));
    o.t2d = clr_value(s2, o.n2, (bad & 0x1fffffull) == 0, hb.flags & BGF_NAN2, lnx);
    o.t1a = clr_value(sa, o.n1a, ((bad >> 21) & 0x1fffffull) == 0, hb.flags & BGF_NAN1A, lnx);
    o.t1b = clr_value(sb, o.n1b, (bad >> 42) == 0, hb.flags & BGF_NAN1B, lnx);
    if (lane == 0) write_rec(out + g, (uint32_t)tk.pool, r, 0u, tk.m, o, bg_zero_flags(hb));
    group_sync<WAVE>();   // every take has landed before the next record's adds
  }
}

// The block null: see the head of this file.  b = min(block, m) (any block >= m is one run of m SNPs, and
// b <= m keeps the real modulo to pools smaller than their windows).  A lane's draws of the first
// 2 NULL_KEEP rows stay in registers for the take pass; later rows are walked again from the saved state.
template <bool P16, bool CNT>
__global__ __launch_bounds__(NULL_MAX_WAVES* WAVE) void k_null_blk(KParams P, const uint32_t* __restrict__ src,
                                                                   const NullTask* __restrict__ tasks, uint32_t R,
                                                                   unsigned long long nrec, uint2 key, uint32_t block,
                                                                   const PL* __restrict__ tab,
                                                                   const BgHead* __restrict__ head, int bg_per_chrom,
                                                                   const double* __restrict__ lnx,
                                                                   sfs2d_window* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const int h2w = P16 ? (P.nb2 + 1) / 2 : P.nb2;
  const int per = null_wave_words(P.nb2, P.n1p, P.n2p, P16);
  uint32_t* H2 = lds + (size_t)wv * per;
  uint32_t* H1a = H2 + h2w;
  uint32_t* H1b = H1a + (P.n1p + 1);
  for (int k = lane; k < per; k += WAVE) H2[k] = 0u;
  group_sync<WAVE>();
  for (unsigned long long g = (unsigned long long)blockIdx.x * nwv + wv; g < nrec; g += (unsigned long long)gridDim.x * nwv) {
    const uint32_t t = (uint32_t)(g / R), r = (uint32_t)(g - (unsigned long long)t * R);
    const NullTask tk = tasks[t];
    const int bg = bg_per_chrom ? tk.pool : 0;
    const TabGlobal T{tab + (size_t)bg * P.nt};
    const BgHead hb = head[bg];
    const bool floatv = hb.flags & BGF_FLOATV;
    const uint32_t b = min(block, tk.m);
    const uint32_t nrow = ((tk.m - 1u) >> 6) + 1u;             // rows of 64 draws
    const uint32_t db = (uint32_t)WAVE / b, eb = (uint32_t)WAVE % b;   // a row on: (j / b, j mod b) += (db, eb)
    const uint32_t rpr = b >= (1u << 26) ? (1u << 27) : 2u * b;        // rows per round (nrow <= 2^26)
    const bool round_pool = b > tk.n;                          // a block longer than the pool goes round it
    // the walk over the rows: ib = this lane's block of the current row, counted from the round's first
    // (+ 128 until the row's round is entered), kb = its place in the block; se / so = the starts of blocks
    // 2 lane and 2 lane + 1 of round rd - 1; left = rows until the next round (all three wave-uniform)
    uint32_t ib = (uint32_t)lane / b + 2u * WAVE, kb = (uint32_t)lane % b, se = 0u, so = 0u;
    uint32_t rd = 0u, left = 0u;
    auto starts = [&](uint32_t round) {
      const uint4 c = philox4x32(make_uint4((uint32_t)WAVE * round + (uint32_t)lane, r, tk.m, (uint32_t)(tk.pool + 1)), key);
      se = null_index(c.x, c.y, 0u, tk.n);
      so = null_index(c.z, c.w, 0u, tk.n);
    };
    auto enter = [&]() {   // before a row: into its round
      if (left == 0u) {
        starts(rd);
        ++rd;
        left = rpr;
        ib -= 2u * WAVE;
      }
      --left;
    };
    // the SNP word of this lane's draw of row `row` (0 -- a word that counts nowhere -- past m), and a row on
    auto word = [&](uint32_t row) -> uint32_t {
      const int from = (int)((ib >> 1) & (uint32_t)(WAVE - 1));
      const uint32_t s0 = (uint32_t)__shfl((int)se, from, WAVE), s1 = (uint32_t)__shfl((int)so, from, WAVE);
      uint32_t w = 0u;
      if (row * (uint32_t)WAVE + (uint32_t)lane < tk.m) {
        uint32_t k = kb;
        if (round_pool) k %= tk.n;
        unsigned long long x = (unsigned long long)((ib & 1u) ? s1 : s0) + k;   // < 2 n
        if (x >= tk.n) x -= tk.n;
        w = snp_word<CNT>(P, src, tk.lo + (uint32_t)x);
      }
      kb += eb;
      ib += db;
      if (kb >= b) { kb -= b; ++ib; }
      return w;
    };
    uint32_t c_var = 0, c2 = 0, c_last = 0, c1a = 0, c1b = 0;
    auto add = [&](uint32_t w) {
      const uint32_t k2 = bin_k2(w), g1 = bin_g1(w), g2 = bin_g2(w);
      c_var += (w & B_VAR) ? 1u : 0u;
      c_last += (w & B_LAST) ? 1u : 0u;
      if (k2) { ++c2; h2_add<P16>(H2, k2); }
      if (g1) { ++c1a; atomicAdd(&H1a[g1], 1u); }
      if (g2) { ++c1b; atomicAdd(&H1b[g2], 1u); }
    };
    uint32_t kw[2 * NULL_KEEP];
#pragma unroll
    for (int i = 0; i < 2 * NULL_KEEP; ++i) {
      kw[i] = 0u;
      if ((uint32_t)i < nrow) {
        if ((i & 1) == 0) enter();   // (a round is 2 b rows: it begins on an even row)
        else --left;
        kw[i] = word((uint32_t)i);
        add(kw[i]);
      }
    }
    const uint32_t ib_k = ib, kb_k = kb, rd_k = rd, left_k = left;   // the walk after the kept rows
    for (uint32_t row = 2 * NULL_KEEP; row < nrow; ++row) {
      enter();
      add(word(row));
    }
    group_sync<WAVE>();
    const unsigned long long r0 = wave_sum_u64((unsigned long long)c2 | ((unsigned long long)c_last << 32));
    const unsigned long long r1 = wave_sum_u64((unsigned long long)c1a | ((unsigned long long)c1b << 32));
    WinOut o;
    o.n2 = (uint32_t)r0;
    o.n2_all = o.n2 + (uint32_t)(r0 >> 32);
    o.n1a = (uint32_t)r1;
    o.n1b = (uint32_t)(r1 >> 32);
    o.snp_count = wave_sum_u(c_var);
    const double N2 = (double)o.n2, N1a = (double)o.n1a, N1b = (double)o.n1b;
    double s2 = 0.0, sa = 0.0, sb = 0.0;
    bool q2 = true, qa = true, qb = true;   // x_k/N == p_k bitwise on every touched bin (eval_exact)
    auto take = [&](uint32_t w) {
      const uint32_t k2 = bin_k2(w), g1 = bin_g1(w), g2 = bin_g2(w);
      if (k2) {
        const uint32_t x = h2_take<P16>(H2, k2);
        if (x) {
          const PL e = T.at(k2);
          s2 += (double)x * (lnx_of(lnx, x) - e.lp);
          q2 &= prop_ok(x, N2, e.v, hb.B2, floatv);
        }
      }
      if (g1) {
        const uint32_t x = atomicExch(&H1a[g1], 0u);
        if (x) {
          const PL e = T.at(P.t1a + g1);
          sa += (double)x * (lnx_of(lnx, x) - e.lp);
          qa &= prop_ok(x, N1a, e.v, hb.B1a, floatv);
        }
      }
      if (g2) {
        const uint32_t x = atomicExch(&H1b[g2], 0u);
        if (x) {
          const PL e = T.at(P.t1b + g2);
          sb += (double)x * (lnx_of(lnx, x) - e.lp);
          qb &= prop_ok(x, N1b, e.v, hb.B1b, floatv);
        }
      }
    };
#pragma unroll
    for (int i = 0; i < 2 * NULL_KEEP; ++i) take(kw[i]);
    if (nrow > 2u * NULL_KEEP) {   // the same draws again: nothing of a replicate window is staged in memory
      ib = ib_k; kb = kb_k; rd = rd_k; left = left_k;
      if (left) starts(rd - 1u);   // (the add pass went on to later rounds)
      for (uint32_t row = 2 * NULL_KEEP; row < nrow; ++row) {
        enter();
        take(word(row));
      }
    }
    s2 = wave_sum_d(s2);
    sa = wave_sum_d(sa);
    sb = wave_sum_d(sb);
    const unsigned long long bad = wave_sum_u64((unsigned long long)(!q2) | ((unsigned long long)(!qa) << 21) |
                                                ((unsigned long long)(!qb) << 42));
    o.t2d = clr_value(s2, o.n2, (bad & 0x1fffffull) == 0, hb.flags & BGF_NAN2, lnx);
    o.t1a = clr_value(sa, o.n1a, ((bad >> 21) & 0x1fffffull) == 0, hb.flags & BGF_NAN1A, lnx);
    o.t1b = clr_value(sb, o.n1b, (bad >> 42) == 0, hb.flags & BGF_NAN1B, lnx);
    if (lane == 0) write_rec(out + g, (uint32_t)tk.pool, r, 0u, tk.m, o, bg_zero_flags(hb));
    group_sync<WAVE>();   // every take has landed before the next record's adds
  }
}

// a sliced plan's tables after a run: k_bg_slice (tail == 0) left table, leaf sums, 1D results and the
// run's inner 2D sums (bcount: the run's parity); this is its tail for every chromosome
__global__ __launch_bounds__(KBLOCK) void k_null_tail(KParams P, const uint32_t* __restrict__ bcount, PL* __restrict__ tab,
                                                      double* __restrict__ LPg, BgHead* __restrict__ head,
                                                      const double* __restrict__ leafsum, const Bg1D* __restrict__ bg1d,
                                                      int nleaves, const int4* __restrict__ nodes, int nnodes,
                                                      int nlevels) {
  __shared__ double node[2 * PW_MAX_LEAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  int4 nd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tid + r * KBLOCK;
    nd[r] = i < nnodes ? nodes[i] : make_int4(0, 0, -1, 0);
    if (i < nleaves) node[i] = leafsum[(size_t)b * nleaves + i];
  }
  __syncthreads();
  for (int l = 0; l < nlevels; ++l) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (nd[r].z == l) node[nleaves + tid + r * KBLOCK] = node[nd[r].x] + node[nd[r].y];
    __syncthreads();
  }
  if (tid == 0) {
    const double B2 = (double)bcount[b];
    const Bg1D o = bg1d[b];
    uint32_t flags = o.flags;
    if (B2 == 0.0) flags |= BGF_B2_ZERO;
    const int M2 = P.nb2 - 2;
    if (M2 >= 1 && B2 != 0.0) {
      const double S = (nleaves + nnodes) ? node[nleaves + nnodes - 1] : 0.0;
      flags |= adjust_last(tab + (size_t)b * P.nt, LPg + (size_t)b * P.nt, M2, 1.0 - S, BGF_NAN2);
    }
    BgHead h;
    h.B2 = B2; h.B1a = o.B1a; h.B1b = o.B1b; h.flags = flags; h.pad = 0;
    head[b] = h;
  }
}
