// sfs2d_projnull.hpp -- the null of the projected scan (included by sfs2d.hip after sfs2d_projscan.hpp).
//
// Replicates of chosen records of a plan's last run in which every used SNP of the window is replaced by a SNP
// drawn from the used SNPs of its chromosome that have the SAME called counts (n1c, n2c):
// the projected T still depends on how close a window's called counts sit to the projection (m1, m2), so a null
// that keeps each window's called counts is the one that can judge it.  Membership, "used" (member & n1c >= m1 &
// n2c >= m2), the weights, the per-term rounding at 2^-e, the joint fold, the three statistics and their NaN / +inf
// rules are section 19's (sfs2d_projscan.hpp), unchanged.
//   pool      of chromosome c: its used SNPs
//   stratum   of a used SNP: the pool's SNPs with the same (n1c, n2c), in ascending SNP index; never empty (the
//             SNP itself is in it)
//   entry     a record index s of the last run; each entry gets R replicates, output record t R + r
//   slot i    of replicate r: SNP k = begin + i of the record's clamped range.  A SNP that is not used draws
//             nothing; a used one with stratum (start, size):
//               c = philox4x32((i >> 1, r, s, chrom + 1), (seed lo, seed hi));
//               x64 = c.x | c.y << 32 (i even), c.z | c.w << 32 (i odd);
//               drawn SNP = pool_idx[start + mulhi64(x64, size)]
//             -- integers only, a function of (seed, s, r, i) and the data (sfs2d.projnull.conditional_draws is
//             the host twin)
//   record    what k_proj_scan would write for a window made of the drawn SNPs against the record's chromosome;
//             n_used / n_dropped are the window's
//   thin      per entry, the used slots whose stratum holds fewer than SFS2D_PNULL_THIN SNPs
// The per-SNP arithmetic of proj_walk and the reduction of k_proj_scan are COPIED here, not shared: the existing
// kernels keep their source and their instruction streams.
#pragma once

#include "sfs2d_projscan.hpp"

namespace sfs2dk {

constexpr uint32_t PNULL_THIN = 8;          // SFS2D_PNULL_THIN

// the dense stratum table: cell ((chrom D1) + (n1c - m1)) D2 + (n2c - m2), D_k = max called count - m_k + 1
struct PnullDims {
  uint32_t d1, d2;
};
__device__ __forceinline__ bool pnull_used(const KParams& P, uint32_t cj, uint32_t wj, uint32_t m1, uint32_t m2,
                                           PnullDims D, bool& member, uint32_t& cell_in_chrom) {
  member = (bin_k2(wj) != 0u) | ((wj & B_LAST) != 0u);
  const uint32_t n1c = (cj & 0xffu) + ((cj >> 8) & 0xffu), n2c = ((cj >> 16) & 0xffu) + (cj >> 24);
  const bool used = member & (n1c >= m1) & (n2c >= m2);
  const uint32_t x1 = n1c - m1, x2 = n2c - m2;
  cell_in_chrom = x1 * D.d2 + x2;
  // (the table covers the data set's largest called counts: a used SNP is always inside it)
  return used & (x1 < D.d1) & (x2 < D.d2);
}

// Pool build, step 1: key[k] = the stratum cell of SNP k (none = the cell count: not used, sorts last), val[k] = k.
// The chromosome by binary search in the nchrom + 1 offsets.
template <bool CNT>
__global__ __launch_bounds__(256) void k_pnull_keys(KParams P, const uint32_t* __restrict__ counts,
                                                    const uint32_t* __restrict__ bins,
                                                    const long long* __restrict__ chrom_off, uint32_t nchrom,
                                                    uint32_t nsnp, uint32_t m1, uint32_t m2, PnullDims D, uint32_t none,
                                                    uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= nsnp) return;
  const uint32_t cj = counts[k];
  const uint32_t wj = CNT ? cls_word(P, cj) : bins[k];
  bool member;
  uint32_t cell;
  const bool used = pnull_used(P, cj, wj, m1, m2, D, member, cell);
  uint32_t lo = 0u, hi = nchrom;   // the last c with chrom_off[c] <= k
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((long long)k >= chrom_off[mid]) lo = mid;
    else hi = mid;
  }
  key[k] = used ? lo * (D.d1 * D.d2) + cell : none;
  val[k] = k;
}

// Pool build, step 3 (after the stable sort by key): segment heads and tails.  phase 0: tab[key].x = the
// segment's first position; phase 1 (a launch of its own): tab[key].y = its length.
__global__ __launch_bounds__(256) void k_pnull_heads(const uint32_t* __restrict__ key, uint32_t nsnp, uint32_t ncell,
                                                     uint2* __restrict__ tab, int phase) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nsnp) return;
  const uint32_t kk = key[i];
  if (kk >= ncell) return;   // (in no pool)
  if (phase == 0) {
    if (i == 0u || key[i - 1u] != kk) tab[kk].x = i;
  } else {
    if (i + 1u == nsnp || key[i + 1u] != kk) tab[kk].y = i + 1u - tab[kk].x;
  }
}

// Workgroup b takes the output records [b nout / G, (b + 1) nout / G), nout = nent R; record g is replicate r = g
// mod R of entry t = g / R, the record s = sel[t] (sel null: t) of the last run.  k_proj_scan's mapping and record
// body; the difference is where a lane's SNP comes from.  Per block of PROJ_ROWS rows of 256 slots, stage by stage
// so that each stage's loads of all rows are in flight together:
//   A   the window SNP's counts word (filtered plans: and its bins word)
//   B   used / dropped, the ballots; the stratum (start, size) from the table in global memory (L2-resident)
//   C   one Philox call per lane and PAIR of rows: slots 2q and 2q + 1 (lanes 2l, 2l + 1 of one row) share a call,
//       so the even lane makes the call of row j, the odd lane that of row j + 1, and each lane takes the two words
//       of its half from the lane that made its row's call by a quad-permute DPP move; then the gather of pool_idx
//   D   the drawn SNP's counts word (a pool SNP is a used member: its bins word is not needed)
//   E   the walk of the drawn SNP's support rectangle (proj_walk's arithmetic), terms added at the folded index
// then k_proj_scan's two passes, fixed-order sums and the 64-byte record; thin[t] by replicate 0.
template <bool CNT>
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_null(KParams P, const uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ bins,
                                                          const sfs2d_window* __restrict__ recs,
                                                          const uint32_t* __restrict__ sel,
                                                          const double* __restrict__ lft, const double* __restrict__ lp,
                                                          const uint2* __restrict__ tab,
                                                          const uint32_t* __restrict__ pool_idx,
                                                          sfs2d_projstat* __restrict__ out, uint32_t* __restrict__ thin,
                                                          uint32_t nout, uint32_t R, uint2 key, uint32_t nbg,
                                                          uint32_t nsnp, uint32_t m1, uint32_t m2, PnullDims D,
                                                          double scale, double inv_scale, uint32_t e_fx) {
  __shared__ double lf[PROJ_LF + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t w2 = m2 + 1u, ngrid = (m1 + 1u) * w2, roww = ngrid + 2u, lpw = ngrid + (m1 + 1u) + w2;
  const uint32_t m12 = m1 + m2;
  const bool fold = P.fold != 0;
  unsigned long long* H = proj_lds;               // [grid | n_used | n_dropped]
  unsigned long long* A1 = H + roww;              // folded marginal of population 1, m1 + 1
  unsigned long long* A2 = A1 + (m1 + 1u);        // ... of population 2, m2 + 1
  unsigned long long* acc = A2 + w2;              // N, N1a, N1b, thin slots (k_proj_scan's spare word)
  double* red = reinterpret_cast<double*>(acc + PSCAN_ACC);   // [wavefront][t2d, t1d_p1, t1d_p2]
  for (uint32_t k = tid; k < PROJ_LF; k += PROJ_BLOCK) lf[k] = lft[k];
  for (uint32_t k = tid; k < roww + (m1 + 1u) + w2 + PSCAN_ACC; k += PROJ_BLOCK) H[k] = 0ull;
  __syncthreads();
  const uint32_t lo = (uint32_t)((unsigned long long)blockIdx.x * nout / gridDim.x);
  const uint32_t hi = (uint32_t)((unsigned long long)(blockIdx.x + 1u) * nout / gridDim.x);
  const bool in1 = tid >= 1u && 2u * tid < m1, in2 = tid >= 1u && 2u * tid < m2;
  const uint32_t cells = D.d1 * D.d2;
  for (uint32_t g = lo; g < hi; ++g) {
    // (the record is the workgroup's: scalar values, uniform branches around the barriers)
    const uint32_t t = g / R, r = g - t * R;
    const uint32_t s = sel ? __builtin_amdgcn_readfirstlane(sel[t]) : t;
    const RecRange rr = rec_range<true>(recs, s, nsnp);
    const uint32_t rflags = rr.flags, b = rr.b, e = rr.e;
    if (rflags) {   // no window of its own: the flags alone
      if (tid == 0) {
        sfs2d_projstat z = {};
        z.flags = rflags;
        out[g] = z;
        if (r == 0u) thin[t] = 0u;
      }
      continue;
    }
    const uint32_t c = __builtin_amdgcn_readfirstlane(recs[s].chrom);
    const uint32_t cbase = c * cells;
    for (uint32_t r0 = b; r0 < e; r0 += PROJ_ROWS * PROJ_BLOCK) {
      uint32_t cw[PROJ_ROWS], w[PROJ_ROWS], cell[PROJ_ROWS], ix[PROJ_ROWS];
      uint2 st[PROJ_ROWS];
      bool used[PROJ_ROWS];
      // A (every lane loads: past the range its last SNP again, dropped by a select)
#pragma unroll
      for (int j = 0; j < PROJ_ROWS; ++j) {
        const uint32_t k = r0 + PROJ_BLOCK * j + tid, kc = min(k, e - 1u);
        const uint32_t cv = counts[kc];
        cw[j] = k < e ? cv : 0u;
        if (!CNT) {
          const uint32_t wv = bins[kc];
          w[j] = k < e ? wv : 0u;
        }
      }
      // B
      uint32_t nt = 0u;
#pragma unroll
      for (int j = 0; j < PROJ_ROWS; ++j) {
        const uint32_t wj = CNT ? cls_word(P, cw[j]) : w[j];
        bool member;
        used[j] = pnull_used(P, cw[j], wj, m1, m2, D, member, cell[j]);
        const uint32_t nu = (uint32_t)__popcll(__ballot(used[j])), nd = (uint32_t)__popcll(__ballot(member & !used[j]));
        if ((tid & (WAVE - 1)) == 0) {
          if (nu) atomicAdd(H + ngrid, (unsigned long long)nu);
          if (nd) atomicAdd(H + ngrid + 1u, (unsigned long long)nd);
        }
        st[j] = tab[used[j] ? cbase + cell[j] : 0u];   // (a lane without a draw reads cell 0: no branch)
      }
      // C
#pragma unroll
      for (int j = 0; j < PROJ_ROWS; j += 2) {
        // slot of this lane in row j (+ 256 for row j + 1); i is even exactly when tid is
        const uint32_t i0 = r0 - b + PROJ_BLOCK * j + tid;
        const uint32_t q = ((tid & 1u) ? i0 + PROJ_BLOCK : i0) >> 1;
        const uint4 cc = philox4x32(make_uint4(q, r, s, c + 1u), key);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          // row j's calls sit on the even lanes (quad_perm [0,0,2,2]), row j + 1's on the odd ones ([1,1,3,3])
          uint32_t xl, xh, zl, zh;
          if (jj == 0) {
            xl = dpp_u<0xA0>(cc.x); xh = dpp_u<0xA0>(cc.y); zl = dpp_u<0xA0>(cc.z); zh = dpp_u<0xA0>(cc.w);
          } else {
            xl = dpp_u<0xF5>(cc.x); xh = dpp_u<0xF5>(cc.y); zl = dpp_u<0xF5>(cc.z); zh = dpp_u<0xF5>(cc.w);
          }
          const uint32_t vl = (tid & 1u) ? zl : xl, vh = (tid & 1u) ? zh : xh;
          const uint2 sj = st[j + jj];
          const uint32_t at = null_index(vl, vh, sj.x, sj.y);   // start + mulhi64(x64, size)
          ix[j + jj] = pool_idx[min(at, nsnp - 1u)];
          nt += (used[j + jj] && sj.y < PNULL_THIN) ? 1u : 0u;
        }
      }
      // D
#pragma unroll
      for (int j = 0; j < PROJ_ROWS; ++j) cw[j] = counts[min(ix[j], nsnp - 1u)];
      // E
#pragma unroll
      for (int j = 0; j < PROJ_ROWS; ++j) {
        if (used[j]) {
          const uint32_t cj = cw[j];
          const uint32_t r1 = cj & 0xffu, a1 = (cj >> 8) & 0xffu, r2 = (cj >> 16) & 0xffu, a2 = cj >> 24;
          const uint32_t n1c = r1 + a1, n2c = r2 + a2;   // (the stratum's: >= m_k, < PROJ_LF)
          if (n1c >= m1 && n2c >= m2) {   // (always: a pool SNP is used)
            const uint32_t l1 = m1 > r1 ? m1 - r1 : 0u, h1 = min(m1, a1);
            const uint32_t l2 = m2 > r2 ? m2 - r2 : 0u, h2 = min(m2, a2);
            const double c1 = proj_lnc(lf, n1c, a1, m1), c2 = proj_lnc(lf, n2c, a2, m2);
            for (uint32_t j1 = l1; j1 <= h1; ++j1) {
              const double v1 = proj_w(lf, c1, n1c, a1, m1, j1) * scale;
              for (uint32_t j2 = l2; j2 <= h2; ++j2) {
                const unsigned long long tm = (unsigned long long)__double2ll_rn(v1 * proj_w(lf, c2, n2c, a2, m2, j2));
                if (tm) {
                  const uint32_t k = j1 * w2 + j2;   // (j1 <= m1, j2 <= m2: inside the grid, and so is its mirror)
                  atomicAdd(H + ((fold && 2u * (j1 + j2) > m12) ? ngrid - 1u - k : k), tm);
                }
              }
            }
          }
        }
      }
      if (r == 0u && nt) atomicAdd(&acc[3], (unsigned long long)nt);
    }
    __syncthreads();   // (every wavefront's adds are in)
    // pass 1
    unsigned long long part = 0ull;
    for (uint32_t k = tid; k < ngrid; k += PROJ_BLOCK) {
      const unsigned long long v = H[k];
      if (v) {
        const uint32_t j1 = k / w2, j2 = k - j1 * w2;
        if (k >= 1u && k + 1u < ngrid) part += v;
        atomicAdd(&A1[min(j1, m1 - j1)], v);
        atomicAdd(&A2[min(j2, m2 - j2)], v);
      }
    }
    if (part) atomicAdd(&acc[0], part);
    __syncthreads();
    if (in1 && A1[tid]) atomicAdd(&acc[1], A1[tid]);
    if (in2 && A2[tid]) atomicAdd(&acc[2], A2[tid]);
    __syncthreads();
    // pass 2
    const unsigned long long N2 = acc[0], N1a = acc[1], N1b = acc[2];
    const bool have_bg = c < nbg;   // (the library's tables hold the record's chromosome: always)
    const double* lpc = lp + (size_t)(have_bg ? c : 0u) * lpw;
    const double lnN = pscan_ln(N2);
    double t2 = 0.0, ta = 0.0, tb = 0.0;
    for (uint32_t k = tid; k < ngrid; k += PROJ_BLOCK) {
      const unsigned long long v = H[k];
      if (v) {
        if (k >= 1u && k + 1u < ngrid) t2 += (double)v * ((pscan_ln(v) - lnN) - lpc[k]);
        H[k] = 0ull;
      }
    }
    if (tid <= m1) {
      const unsigned long long v = A1[tid];
      if (in1 && v) ta = (double)v * ((pscan_ln(v) - pscan_ln(N1a)) - lpc[ngrid + tid]);
      A1[tid] = 0ull;
    }
    if (tid <= m2) {
      const unsigned long long v = A2[tid];
      if (in2 && v) tb = (double)v * ((pscan_ln(v) - pscan_ln(N1b)) - lpc[ngrid + m1 + 1u + tid]);
      A2[tid] = 0ull;
    }
    t2 = wave_sum_dpp(t2);
    ta = wave_sum_dpp(ta);
    tb = wave_sum_dpp(tb);
    if ((tid & (WAVE - 1)) == 0) {
      double* rd = red + 3u * (tid / WAVE);
      rd[0] = t2; rd[1] = ta; rd[2] = tb;
    }
    __syncthreads();
    if (tid == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      const double s2 = ((red[0] + red[3]) + red[6]) + red[9];
      const double sa = ((red[1] + red[4]) + red[7]) + red[10];
      const double sb = ((red[2] + red[5]) + red[8]) + red[11];
      sfs2d_projstat o;
      o.t2d = (N2 && have_bg) ? 2.0 * s2 * inv_scale : nan;
      o.t1d_p1 = (N1a && have_bg) ? 2.0 * sa * inv_scale : nan;
      o.t1d_p2 = (N1b && have_bg) ? 2.0 * sb * inv_scale : nan;
      o.n2_fx = (long long)N2;
      o.n1a_fx = (long long)N1a;
      o.n1b_fx = (long long)N1b;
      o.n_used = (uint32_t)H[ngrid];
      o.n_dropped = (uint32_t)H[ngrid + 1u];
      o.flags = 0u;
      o.e = e_fx;
      out[g] = o;
      if (r == 0u) thin[t] = (uint32_t)acc[3];
      H[ngrid] = H[ngrid + 1u] = 0ull;
      acc[0] = acc[1] = acc[2] = acc[3] = 0ull;
    }
    __syncthreads();   // (the grid, the marginals and the accumulators are empty again)
  }
}

}  // namespace sfs2dk
