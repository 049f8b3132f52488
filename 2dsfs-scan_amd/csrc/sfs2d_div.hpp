// sfs2d_div.hpp -- per-window diversity sums (included by sfs2d.hip after sfs2d_kernels.hpp).
//
// What kind of window a T2D / Fst peak is: nucleotide diversity of each population (pi), absolute divergence
// (dxy), Watterson's theta and the inputs of Tajima's D, as sums over the window's SNPs of functions of the
// SNP's four allele counts.  Per SNP of the window's 2D SFS (the SNPs the SFS drops as
// bin (0, 0) are fixed for one allele in both populations: every term below is exactly 0 for them), with
// population k's counts (r, a), n = r + a:
//   pi_k      2 a r / (n (n - 1))             n >= 2, else 0; the integer a r first: a fixed site adds exactly 0.0
//   S_k       1 when 0 < a < n                (then n >= 2)
//   thw_k     S_k / h(n),  h(n) = sum_{i=1}^{n-1} 1 / i
//   dxy       (a1 r2 + r1 a2) / (n1 n2)       n1, n2 >= 1, else 0; the integer numerator first
//   fully called in k: n == 2 pop_size_k exactly: S_full,k and AR_full,k = sum a r (u64) -- Tajima's D is formed
//   from them on the host (one sample size).
// All fields of a record are sums over the window; per-site values are formed on the host.
#pragma once

#include "sfs2d_kernels.hpp"

namespace sfs2dk {

static_assert(sizeof(sfs2d_diversity) == 80, "diversity record must be 80 bytes");

constexpr int DIV_BLOCK = 256;   // k_div_win workgroup: four wavefronts, a record each
constexpr int DIV_ROWS = 8;      // rows of 64 SNPs whose loads are in flight together

// u64 wave sum on the DPP path (wave_sum_dpp's steps on integers: exact, any order gives the same sum)
__device__ __forceinline__ unsigned long long wave_sum_dpp_u64(unsigned long long v) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  // the low words' sum can carry: sum the 16-bit halves of the low word apart (64 lanes x 2^16 < 2^32)
  const uint32_t l0 = wave_sum_dpp_u(lo & 0xffffu), l1 = wave_sum_dpp_u(lo >> 16), h = wave_sum_dpp_u(hi);
  return (unsigned long long)l0 + ((unsigned long long)l1 << 16) + ((unsigned long long)h << 32);
}

// One wavefront per record of the last run (records wave_id, wave_id + nwaves, ...): the window's SNP range
// [begin, end) from the record itself (not from the slot table: k_scan_w clears slots, index plans write theirs
// once), membership as fst_windows takes it (the packed bins of a filtered plan, cls_word of the counts on a
// counts plan), per-lane fp64 and integer sums in row order, one DPP reduction per field (deterministic), the
// 80-byte record stored by lane 0.  rt: (1/n, 1/(n(n-1))), hw: 1/h(n), both in LDS, 0 below n = 2.
template <bool CNT>
__device__ __forceinline__ void div_windows(const KParams& P, const uint32_t* __restrict__ counts,
                                            const uint32_t* __restrict__ bins, const sfs2d_window* __restrict__ recs,
                                            const double2* rt, const double* hw, sfs2d_diversity* __restrict__ out,
                                            uint32_t nrec, uint32_t nsnp, uint32_t wave_id, uint32_t nwaves) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (uint32_t s = wave_id; s < nrec; s += nwaves) {
    const RecRange rr = rec_range<false>(recs, s, nsnp);
    const uint32_t rf = rr.flags, b = rr.b, e = rr.e;
    sfs2d_diversity o;
    memset(&o, 0, sizeof(o));
    o.flags = rf;
    if (rf) {   // no window of its own: flagged, every sum 0
      if (lane == 0) out[s] = o;
      continue;
    }
    double pi1 = 0.0, pi2 = 0.0, dxy = 0.0, th1 = 0.0, th2 = 0.0;
    unsigned long long af1 = 0, af2 = 0;
    uint32_t s1 = 0, s2 = 0, f1 = 0, f2 = 0;
    for (uint32_t r0 = b; r0 < e; r0 += DIV_ROWS * WAVE) {
      uint32_t c[DIV_ROWS], w[DIV_ROWS];
#pragma unroll
      for (int j = 0; j < DIV_ROWS; ++j) {
        // (every lane loads: past the window's end its last SNP again, then dropped -- no branch around a load)
        const uint32_t i = r0 + WAVE * j + lane, ic = min(i, e - 1u);
        const uint32_t cv = counts[ic];
        c[j] = i < e ? cv : 0u;
        if (!CNT) {
          const uint32_t wv = bins[ic];
          w[j] = i < e ? wv : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < DIV_ROWS; ++j) {
        const uint32_t wj = CNT ? cls_word(P, c[j]) : w[j];   // (counts 0 past e: outside the set)
        const bool member = (bin_k2(wj) != 0u) | ((wj & B_LAST) != 0u);
        const uint32_t cj = member ? c[j] : 0u;
        const uint32_t r1 = cj & 0xffu, a1 = (cj >> 8) & 0xffu, r2 = (cj >> 16) & 0xffu, a2 = cj >> 24;
        const uint32_t n1c = r1 + a1, n2c = r2 + a2;   // u8 counts: n <= 510 < RCPN
        const uint32_t ar1 = __umul24(a1, r1), ar2 = __umul24(a2, r2);
        const double2 q1 = rt[n1c], q2 = rt[n2c];
        pi1 += (double)(2u * ar1) * q1.y;
        pi2 += (double)(2u * ar2) * q2.y;
        // 1/n for dxy holds from n = 1 on (the table is 0 below 2)
        const double i1 = n1c == 1u ? 1.0 : q1.x, i2 = n2c == 1u ? 1.0 : q2.x;
        dxy += (double)(__umul24(a1, r2) + __umul24(r1, a2)) * (i1 * i2);
        const bool g1 = ar1 != 0u, g2 = ar2 != 0u;   // segregating: 0 < a < n
        const double h1 = hw[n1c], h2 = hw[n2c];
        th1 += g1 ? h1 : 0.0;
        th2 += g2 ? h2 : 0.0;
        s1 += g1;
        s2 += g2;
        const bool u1 = n1c == (uint32_t)P.n1, u2 = n2c == (uint32_t)P.n2;   // fully called
        f1 += g1 & u1;
        f2 += g2 & u2;
        af1 += u1 ? ar1 : 0u;
        af2 += u2 ? ar2 : 0u;
        // a row's table reads stay with its row: with all eight rows' table values live at once the kernel
        // took 180 VGPRs (two wavefronts per SIMD) instead of 58-66
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    o.pi1 = wave_sum_dpp(pi1);
    o.pi2 = wave_sum_dpp(pi2);
    o.dxy = wave_sum_dpp(dxy);
    o.thw1 = wave_sum_dpp(th1);
    o.thw2 = wave_sum_dpp(th2);
    o.ar1_full = wave_sum_dpp_u64(af1);
    o.ar2_full = wave_sum_dpp_u64(af2);
    o.s1 = wave_sum_dpp_u(s1);
    o.s2 = wave_sum_dpp_u(s2);
    o.s1_full = wave_sum_dpp_u(f1);
    o.s2_full = wave_sum_dpp_u(f2);
    if (lane == 0) out[s] = o;
  }
}

template <bool CNT>
__global__ __launch_bounds__(DIV_BLOCK) void k_div_win(KParams P, const uint32_t* __restrict__ counts,
                                                       const uint32_t* __restrict__ bins,
                                                       const sfs2d_window* __restrict__ recs,
                                                       const double2* __restrict__ rt, const double* __restrict__ hwt,
                                                       sfs2d_diversity* __restrict__ out, uint32_t nrec,
                                                       uint32_t nsnp) {
  __shared__ double2 rl[RCPN];   // (1/n, 1/(n(n-1))), as k_fst_win
  __shared__ double hl[RCPN];    // 1/h(n)
  for (int k = threadIdx.x; k < RCPN; k += DIV_BLOCK) {
    rl[k] = rt[k];
    hl[k] = hwt[k];
  }
  __syncthreads();
  div_windows<CNT>(P, counts, bins, recs, rl, hl, out, nrec, nsnp,
                   blockIdx.x * (DIV_BLOCK / WAVE) + (threadIdx.x >> 6),
                   gridDim.x * (DIV_BLOCK / WAVE));
}

}  // namespace sfs2dk
