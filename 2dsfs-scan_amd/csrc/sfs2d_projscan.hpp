// sfs2d_projscan.hpp -- the projected scan (included by sfs2d.hip after sfs2d_proj.hpp).
//
// T2D and T1D of EVERY record of a plan's last run at a common sample size (m1, m2): the
// window's projected joint spectrum (section 18: members, used and dropped SNPs, the weights h(j; n, a, m), terms
// rounded to nearest once at 2^-e, integer sums) is built in LDS and reduced there against the projected spectrum
// of the window's chromosome; 64 bytes per window reach global memory, no grid does.
//   window grid X   the projected grid of the record's SNP range, folded jointly when the plan folds: bin (j1, j2)
//                   with 2 (j1 + j2) > m1 + m2 goes to (m1 - j1, m2 - j2), a tie stays (spectra.fold_projected);
//                   the fold is applied at add time, as an index map -- the grid is linear in the terms
//   background b    the same grid over the record's chromosome (or one chromosome for every record)
//   T2D             2 sum_{x_k > 0} x_k (ln(x_k / N) - ln(b_k / B)) over x = X.ravel()[1:-1], N = sum x, B = sum
//                   b[1:-1]; +inf when a touched bin has b_k = 0; NaN exactly when N = 0 or B = 0
//   T1D_k           the same form on the folded marginal min(j, m_k - j) of the (folded) grid at its inner bins
//                   1 <= j, 2 j < m_k, against the chromosome's
// The closed form is the statistic: the reference's exact-0.0 identity of proportional spectra and scipy's p[-1]
// NaN rule are not reproduced.
#pragma once

#include "sfs2d_proj.hpp"

namespace sfs2dk {

constexpr int PSCAN_ACC = 4;    // u64 accumulators behind the marginals: N, N1a, N1b (one spare)
constexpr int PSCAN_RED = 12;   // four wavefronts' partial sums of the three statistics

// words of dynamic LDS (8 bytes each): the grid and its two counters (a k_proj_win row), the two folded marginals,
// the accumulators and the partial sums; the 4 KB table of ln k! is static
__host__ __device__ inline size_t pscan_lds_words(uint32_t m1, uint32_t m2) {
  return (size_t)(m1 + 1u) * (m2 + 1u) + 2u + (m1 + 1u) + (m2 + 1u) + PSCAN_ACC + PSCAN_RED;
}

// ln of a fixed-point word, out of line: the reduction's logarithms share one copy of log (as log_u32 in
// sfs2d_kernels.hpp: about 500 instructions and 13 VGPRs fewer per instantiation than inlined; the time is the same)
__device__ __noinline__ double pscan_ln(unsigned long long v) { return log((double)v); }

// the folded value of bin k of an unfolded row g (s = j1 + j2 of the bin): a bin below the anti-diagonal takes its
// mirror's, a tie keeps its own, a bin above is empty
__device__ __forceinline__ unsigned long long pscan_fold_bin(const unsigned long long* __restrict__ g, uint32_t k,
                                                             uint32_t ngrid, uint32_t s, uint32_t m12, bool fold) {
  if (!fold) return g[k];
  if (2u * s > m12) return 0ull;
  return 2u * s < m12 ? g[k] + g[ngrid - 1u - k] : g[k];
}

// One workgroup per background chromosome c: rows[c] is the chromosome's unfolded row from k_proj_win ([grid |
// n_used | n_dropped], fixed point 2^-e_bg, which cancels below).  Writes lp[c] = [ln b_k - ln B, ngrid doubles |
// ln f1_j - ln N1a, m1 + 1 | ln f2_j - ln N1b, m2 + 1]: -inf at an empty bin, NaN when the sum is 0 by itself
// (-inf - -inf); the 1D entries outside the inner bins are 0.  The sums are integer (LDS atomics: any order).
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_lp(const unsigned long long* __restrict__ rows,
                                                        double* __restrict__ lp, uint32_t m1, uint32_t m2, int fold) {
  __shared__ unsigned long long f1[256], f2[256], acc[PSCAN_ACC];
  const uint32_t tid = threadIdx.x;
  const uint32_t w2 = m2 + 1u, ngrid = (m1 + 1u) * w2, roww = ngrid + 2u, lpw = ngrid + (m1 + 1u) + w2;
  const unsigned long long* g = rows + (size_t)blockIdx.x * roww;
  double* o = lp + (size_t)blockIdx.x * lpw;
  f1[tid] = f2[tid] = 0ull;   // (m_k + 1 <= 255 entries)
  if (tid < PSCAN_ACC) acc[tid] = 0ull;
  __syncthreads();
  unsigned long long part = 0ull;
  for (uint32_t k = tid; k < ngrid; k += PROJ_BLOCK) {
    const uint32_t j1 = k / w2, j2 = k - j1 * w2;
    const unsigned long long v = pscan_fold_bin(g, k, ngrid, j1 + j2, m1 + m2, fold != 0);
    if (k >= 1u && k + 1u < ngrid) part += v;
    if (v) {
      atomicAdd(&f1[min(j1, m1 - j1)], v);
      atomicAdd(&f2[min(j2, m2 - j2)], v);
    }
  }
  if (part) atomicAdd(&acc[0], part);
  __syncthreads();
  const bool in1 = tid >= 1u && 2u * tid < m1, in2 = tid >= 1u && 2u * tid < m2;
  if (in1 && f1[tid]) atomicAdd(&acc[1], f1[tid]);
  if (in2 && f2[tid]) atomicAdd(&acc[2], f2[tid]);
  __syncthreads();
  const double lnB = log((double)acc[0]), lnA = log((double)acc[1]), lnC = log((double)acc[2]);
  for (uint32_t k = tid; k < ngrid; k += PROJ_BLOCK) {
    const uint32_t j1 = k / w2, j2 = k - j1 * w2;
    o[k] = log((double)pscan_fold_bin(g, k, ngrid, j1 + j2, m1 + m2, fold != 0)) - lnB;
  }
  if (tid <= m1) o[ngrid + tid] = in1 ? log((double)f1[tid]) - lnA : 0.0;
  if (tid <= m2) o[ngrid + m1 + 1u + tid] = in2 ? log((double)f2[tid]) - lnC : 0.0;
}

// Workgroup b takes the records [b nrec / G, (b + 1) nrec / G).  Per record: the SNP range (rec_range) projected by
// proj_walk, as k_proj_win projects an entry, the terms added with non-returning LDS atomics into the u64 grid at
// the FOLDED index; then, in place:
//   pass 1   the inner sum N (u64, exact) and every bin into the two folded marginals (integer LDS atomics)
//   pass 2   per lane over its bins in index order x_k ((ln x_k - ln N) - lp_k) for x_k > 0, the word zeroed in the
//            same pass (the next record of the workgroup starts from an empty grid); the 1D terms from the marginal
//            accumulators the same way; the fixed-order DPP wave sum, the four wavefronts' partials added in order
// and one 64-byte record stored by thread 0.  The fixed point 2^e cancels inside the logarithms and scales the sums
// once at the end (inv_scale = 2^-e).  Nothing depends on how the records fall to workgroups: two calls give
// byte-equal records.  bg_one: every record against row 0 of lp (one chosen chromosome), else row recs[s].chrom.
template <bool CNT>
__global__ __launch_bounds__(PROJ_BLOCK) void k_proj_scan(KParams P, const uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ bins,
                                                          const sfs2d_window* __restrict__ recs,
                                                          const double* __restrict__ lft, const double* __restrict__ lp,
                                                          sfs2d_projstat* __restrict__ out, uint32_t nrec, uint32_t nbg,
                                                          uint32_t nsnp, uint32_t m1, uint32_t m2, int bg_one,
                                                          double scale, double inv_scale, uint32_t e_fx) {
  __shared__ double lf[PROJ_LF + 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t w2 = m2 + 1u, ngrid = (m1 + 1u) * w2, roww = ngrid + 2u, lpw = ngrid + (m1 + 1u) + w2;
  const uint32_t m12 = m1 + m2;
  const bool fold = P.fold != 0;
  unsigned long long* H = proj_lds;               // [grid | n_used | n_dropped]
  unsigned long long* A1 = H + roww;              // folded marginal of population 1, m1 + 1
  unsigned long long* A2 = A1 + (m1 + 1u);        // ... of population 2, m2 + 1
  unsigned long long* acc = A2 + w2;              // N, N1a, N1b
  double* red = reinterpret_cast<double*>(acc + PSCAN_ACC);   // [wavefront][t2d, t1d_p1, t1d_p2]
  for (uint32_t k = tid; k < PROJ_LF; k += PROJ_BLOCK) lf[k] = lft[k];
  for (uint32_t k = tid; k < roww + (m1 + 1u) + w2 + PSCAN_ACC; k += PROJ_BLOCK) H[k] = 0ull;
  __syncthreads();
  const uint32_t lo = (uint32_t)((unsigned long long)blockIdx.x * nrec / gridDim.x);
  const uint32_t hi = (uint32_t)((unsigned long long)(blockIdx.x + 1u) * nrec / gridDim.x);
  const bool in1 = tid >= 1u && 2u * tid < m1, in2 = tid >= 1u && 2u * tid < m2;
  for (uint32_t s = lo; s < hi; ++s) {
    // (the record is the workgroup's: scalar values, uniform branches around the barriers)
    const RecRange rr = rec_range<true>(recs, s, nsnp);
    const uint32_t rflags = rr.flags, b = rr.b, e = rr.e;
    if (rflags) {   // no window of its own: the flags alone
      if (tid == 0) {
        sfs2d_projstat z = {};
        z.flags = rflags;
        out[s] = z;
      }
      continue;
    }
    const uint32_t c = bg_one ? 0u : __builtin_amdgcn_readfirstlane(recs[s].chrom);
    proj_walk<CNT>(
        P, counts, bins, lf, b, e, m1, m2, scale,
        [&](uint32_t nu, uint32_t nd) {
          if (nu) atomicAdd(H + ngrid, (unsigned long long)nu);
          if (nd) atomicAdd(H + ngrid + 1u, (unsigned long long)nd);
        },
        [&](uint32_t j1, uint32_t j2, unsigned long long t) {
          const uint32_t k = j1 * w2 + j2;   // (j1 <= m1, j2 <= m2: inside the grid, and so is its mirror)
          atomicAdd(H + ((fold && 2u * (j1 + j2) > m12) ? ngrid - 1u - k : k), t);
        });
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
      double* r = red + 3u * (tid / WAVE);
      r[0] = t2; r[1] = ta; r[2] = tb;
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
      out[s] = o;
      H[ngrid] = H[ngrid + 1u] = 0ull;
      acc[0] = acc[1] = acc[2] = 0ull;
    }
    __syncthreads();   // (the grid, the marginals and the accumulators are empty again)
  }
}

}  // namespace sfs2dk
